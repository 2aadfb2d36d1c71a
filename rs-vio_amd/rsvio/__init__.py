"""rsvio -- MI355X-native RS-VIO hot paths (patch tracker + sliding-window BA).

Python host mirror of the reference's Rust API over the C ABI (include/rsvio_gpu.h).
All compute runs in lib/librsvio_gpu.so (HIP, gfx950); there is no CPU fallback.
"""
from ._lib import RsvioError, load, require_device  # noqa: F401
from .motion import PoseCovariance  # noqa: F401
from .tracker import (StereoGate, StereoPatchTracker, TrackerBatch, build_image_pyramid,  # noqa: F401
                      detect_key_points, predict_seeds, pyramid_bytes, pyramid_levels, stereo_gate_lists,
                      track_points, track_points_seeded)

__all__ = ["RsvioError", "load", "require_device", "PoseCovariance", "StereoGate", "StereoPatchTracker",
           "TrackerBatch", "build_image_pyramid", "detect_key_points", "predict_seeds", "pyramid_bytes",
           "pyramid_levels", "stereo_gate_lists", "track_points", "track_points_seeded"]
