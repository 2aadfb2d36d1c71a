"""The batched keyframe step against B single calls on the same handles.

For B in --n (default 1 16 64) windows of config-3 shape (10 keyframes, 2,000 landmarks, 24,000
observations; seeds differ per window), each on its own handle, times on the C ABI with every
argument marshalled beforehand
  triangulate   B rsvio_ba_triangulate (all landmarks, every output asked for: one wait each)
                against one rsvio_ba_batch_triangulate with the same outputs (one wait),
  run           B rsvio_ba_run against one rsvio_ba_batch_run_active (NULL: every window),
  check         B rsvio_ba_check_landmarks against one rsvio_ba_batch_check_landmarks,
  covariance    B rsvio_ba_covariance (every landmark, the per-keyframe blocks) against one
                rsvio_ba_batch_covariance,
in that order inside each repetition, so check and covariance read a solved state.  Wall times are
host clocks around calls that end in a stream synchronise; device_ms is the batched call's
*device_ms (the single covariance's: the sum of its info.device_ms over the windows).  Every figure
is the median of --reps repetitions after --warmup; p10 / p90 give the spread.  Each batched call
is first checked to return the single calls' results bit for bit.  The single calls are the
library's existing entry points: the comparison is at one commit.

usage: python tools/ba_batch_keyframe_probe.py [--n 1 16 64] [--reps 30] [--out profiles/ba_batch_keyframe_probe.json]
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

from rsvio import _lib  # noqa: E402
from rsvio import ba as B  # noqa: E402
from rsvio import synthetic as S  # noqa: E402


def _stats(x):
    x = np.asarray(x, np.float64)
    return dict(median=float(np.median(x)), p10=float(np.percentile(x, 10)), p90=float(np.percentile(x, 90)))


class Legs:
    """The single and batched calls over `wins` with prebuilt arguments and output buffers."""

    def __init__(self, wins):
        lib = self.lib = _lib.load()
        n = self.n = len(wins)
        self.wins, self.batch = wins, B.BundleBatch(wins)
        self.gate, self.cfg = B.landmark_gate(B.TRI_ALL_VIEWS), B.lm_cfg()
        self.ms = C.c_double(0.0)
        self.single_dev_ms = 0.0
        mk = lambda w: dict(pw=np.empty((w.n_lm, 3)), info=np.zeros(w.n_lm, _lib.LANDMARK_INFO_DTYPE),  # noqa: E731
                            cp=np.zeros((w.n_kf, 36)), lm=np.zeros((w.n_lm, 9)), fl=np.zeros(w.n_lm, np.uint8))
        self.s, self.b = [mk(w) for w in wins], [mk(w) for w in wins]
        self.s_n = [C.c_int32(0) for _ in wins]
        self.s_res, self.b_res = (_lib.BaResult * n)(), (_lib.BaResult * n)()
        self.s_cov = [_lib.CovInfo() for _ in wins]
        self.lm_slots, self.cov_slots = (_lib.BaLandmarkSlot * n)(), (_lib.BaCovSlot * n)()
        for w, o, ls, cs in zip(wins, self.b, self.lm_slots, self.cov_slots):
            ls.p_W_out, ls.info_out, ls.n_lm = _lib.ptr(o["pw"]), _lib.ptr(o["info"]), w.n_lm
            cs.cov_pose, cs.cov_lm, cs.lm_flags, cs.n_sel = _lib.ptr(o["cp"]), _lib.ptr(o["lm"]), _lib.ptr(o["fl"]), w.n_lm
        g = C.byref(self.gate)
        self.a_tri = [(w._h, None, w.n_lm, g, _lib.ptr(o["pw"]), _lib.ptr(o["info"]), C.byref(k))
                      for w, o, k in zip(wins, self.s, self.s_n)]
        self.a_run = [(w._h, C.byref(self.cfg), C.byref(self.s_res[i])) for i, w in enumerate(wins)]
        self.a_chk = [(w._h, w.n_lm, g, _lib.ptr(o["info"]), C.byref(k)) for w, o, k in zip(wins, self.s, self.s_n)]
        self.a_cov = [(w._h, 2.0, None, _lib.ptr(o["cp"]), None, w.n_lm, _lib.ptr(o["lm"]), _lib.ptr(o["fl"]),
                       C.byref(i)) for w, o, i in zip(wins, self.s, self.s_cov)]

    def triangulate_single(self):
        for a in self.a_tri:
            _lib.check(self.lib.rsvio_ba_triangulate(*a))

    def triangulate_batch(self):
        _lib.check(self.lib.rsvio_ba_batch_triangulate(self.batch._h, None, C.byref(self.gate), self.lm_slots,
                                                       C.byref(self.ms)))

    def run_single(self):
        for a in self.a_run:
            _lib.check(self.lib.rsvio_ba_run(*a))

    def run_batch(self):
        _lib.check(self.lib.rsvio_ba_batch_run_active(self.batch._h, None, C.byref(self.cfg), self.b_res))
        self.ms.value = self.b_res[0].solve_ms

    def check_single(self):
        for a in self.a_chk:
            _lib.check(self.lib.rsvio_ba_check_landmarks(*a))

    def check_batch(self):
        _lib.check(self.lib.rsvio_ba_batch_check_landmarks(self.batch._h, None, C.byref(self.gate), self.lm_slots,
                                                           C.byref(self.ms)))

    def covariance_single(self):
        for a in self.a_cov:
            _lib.check(self.lib.rsvio_ba_covariance(*a))
        self.single_dev_ms = sum(i.device_ms for i in self.s_cov)

    def covariance_batch(self):
        _lib.check(self.lib.rsvio_ba_batch_covariance(self.batch._h, None, 2.0, self.cov_slots, C.byref(self.ms)))

    def same(self, keys):
        return all(s[k].tobytes() == b[k].tobytes() for s, b in zip(self.s, self.b) for k in keys)

    def verify(self):
        self.triangulate_single(), self.triangulate_batch()
        assert self.same(("pw", "info")) and [k.value for k in self.s_n] == [s.n_ok for s in self.lm_slots]
        self.run_single()
        one = [w.state() for w in self.wins]
        self.run_batch()
        for i, w in enumerate(self.wins):
            assert (self.s_res[i].status, self.s_res[i].iterations) == (self.b_res[i].status, self.b_res[i].iterations)
            assert all(np.abs(x - y).max() <= 1e-10 for x, y in zip(one[i], w.state()))
        self.check_single(), self.check_batch()
        assert self.same(("info",))
        self.covariance_single(), self.covariance_batch()
        assert self.same(("cp", "lm", "fl")) and all(s.info.status == B.COV_OK for s in self.cov_slots)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 30:
        ap.error("--reps must be at least 30")
    n_max = max(a.n)
    wins = []
    for i in range(n_max):
        p = S.ba_problem(seed=7 + 2 * i, init_seed=11 + 2 * i)
        w = B.BundleAdjuster(max_keyframes=p.n_kf, max_landmarks=p.n_lm, max_observations=p.n_obs)
        w.set_problem_from(p)
        wins.append(w)
    rows = []
    calls = ("triangulate", "run", "check", "covariance")
    for n in a.n:
        legs = Legs(wins[:n])
        legs.verify()
        wall = {f"{c}_{k}": [] for c in calls for k in ("single", "batch")}
        dev = {c: [] for c in calls}
        cov_single_dev = []
        for rep in range(a.warmup + a.reps):
            for c in calls:
                for k in ("single", "batch"):
                    fn = getattr(legs, f"{c}_{k}")
                    t0 = time.perf_counter()
                    fn()
                    dt = (time.perf_counter() - t0) * 1e3
                    if rep < a.warmup:
                        continue
                    wall[f"{c}_{k}"].append(dt)
                    if k == "batch":
                        dev[c].append(legs.ms.value)
                    elif c == "covariance":
                        cov_single_dev.append(legs.single_dev_ms)
        row = dict(n=n, reps=a.reps, shape="config 3: 10 keyframes, 2000 landmarks, 24000 observations",
                   wall_ms={k: _stats(v) for k, v in wall.items()},
                   batch_device_ms={k: _stats(v) for k, v in dev.items()},
                   covariance_single_device_ms_sum=_stats(cov_single_dev),
                   gain={c: float(np.median(wall[c + "_single"]) / np.median(wall[c + "_batch"])) for c in calls})
        legs.batch.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
    for w in wins:
        w.close()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
