"""rsvio_track_prediction, rsvio_prediction_counts and the entry points of motion-predicted tracking
without a device: the ctypes structures of rsvio/_lib.py have the size and the member offsets the C
compiler gives include/rsvio_gpu.h's (a small program prints them), the new symbols are declared,
bound, exported and listed in INTEGRATION.md, and the argument checks that need no device answer
before any device call."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
INCLUDE = ROOT / "include"

STRUCTS = {"rsvio_track_prediction": ("TrackPrediction", ["R_l", "R_r"], 144),
           "rsvio_prediction_counts": ("PredictionCounts", ["n_seeded", "n_unseeded"], 16)}
SYMBOLS = ["rsvio_project", "rsvio_project_d", "rsvio_predict_seeds", "rsvio_predict_seeds_d",
           "rsvio_track_points_seeded", "rsvio_tracker_set_prediction", "rsvio_tracker_prediction_report"]


def _c_layout(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rsvio_gpu.h"', "int main(void) {"]
    for c_name, (_, members, _) in STRUCTS.items():
        lines.append(f'  printf("{c_name} %zu\\n", sizeof({c_name}));')
        lines += [f'  printf("{c_name}.{m} %zu\\n", offsetof({c_name}, {m}));' for m in members]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", str(INCLUDE), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_structs_match_the_header(tmp_path):
    from rsvio import _lib
    lay = _c_layout(tmp_path)
    for c_name, (py_name, members, size) in STRUCTS.items():
        T = getattr(_lib, py_name)
        assert [f[0] for f in T._fields_] == members
        assert C.sizeof(T) == lay[c_name] == size
        for m in members:
            assert getattr(T, m).offset == lay[f"{c_name}.{m}"], (c_name, m)


def test_symbols_are_declared_bound_exported_and_documented():
    from rsvio import _lib
    lib = _lib.load()
    header = (INCLUDE / "rsvio_gpu.h").read_text()
    doc = (ROOT / "INTEGRATION.md").read_text()
    for s in SYMBOLS:
        assert s in _lib.SIG
        assert getattr(lib, s).argtypes == _lib.SIG[s][1]
        assert f" {s}(" in header
        assert f"pub fn {s}(" in doc


def test_arguments_are_checked_before_any_device_call():
    from rsvio import _lib
    lib = _lib.load()
    cam = _lib.Camera()
    cam.model, cam.params[0], cam.params[1] = 0, 100.0, 100.0
    eye = np.eye(3)
    # projection: an unknown model, NULL buffers with n > 0; n = 0 is a no-op
    bad = _lib.Camera()
    bad.model = 7
    assert lib.rsvio_project(C.byref(bad), None, 0, None, None) == -1
    assert lib.rsvio_project(C.byref(cam), None, 3, None, None) == -1
    assert lib.rsvio_project(C.byref(cam), None, 0, None, None) == 0
    assert lib.rsvio_project_d(C.byref(cam), None, 0, None, None, None) == 0
    # seeds: a NULL rotation, a non-rotation (scaled, mirrored, NaN) -- refused with n = 0 too
    assert lib.rsvio_predict_seeds(C.byref(cam), None, None, 0, 64, 48, None, None) == -1
    for R in (1.001 * eye, np.diag([1.0, 1.0, -1.0]), np.full((3, 3), np.nan)):
        R = np.ascontiguousarray(R)
        assert lib.rsvio_predict_seeds(C.byref(cam), R.ctypes.data, None, 0, 64, 48, None, None) == -1
        assert b"not a rotation" in lib.rsvio_last_error()
    assert lib.rsvio_predict_seeds(C.byref(cam), eye.ctypes.data, None, 0, 64, 48, None, None) == 0
    assert lib.rsvio_predict_seeds(C.byref(cam), eye.ctypes.data, None, 2, 64, 48, None, None) == -1
    # seeded LK and the handle's calls
    assert lib.rsvio_track_points_seeded(None, None, 10, 10, 1, None, None, 0, 20, C.c_float(0.01), None, None) == -1
    assert lib.rsvio_tracker_set_prediction(None, None) == -1
    assert lib.rsvio_tracker_prediction_report(None, None, None, 0, None, 0) == -1


def test_python_surface():
    import inspect

    from rsvio import StereoPatchTracker, synthetic, tracker
    from rsvio.camera import Camera
    from rsvio.estimator import Estimator, FrameResult, NativeEstimator
    for m in ("set_prediction", "prediction_report", "prediction_counts"):
        assert callable(getattr(StereoPatchTracker, m))
    assert callable(tracker.track_points_seeded) and callable(tracker.predict_seeds) and callable(Camera.project)
    assert callable(synthetic.rotating_scene_pair)
    assert inspect.signature(Estimator.__init__).parameters["predict"].default is None
    assert inspect.signature(Estimator.process_frame).parameters["delta_R_B"].default is None
    assert "n_seeded" in FrameResult.__dataclass_fields__
    try:
        NativeEstimator(None, np.eye(4), np.eye(4), predict="external")
    except ValueError:
        pass
    else:
        raise AssertionError("NativeEstimator accepted predict")
