"""rsvio_ransac_cfg and rsvio_robust_motion_result: the ctypes structures of rsvio/_lib.py have the
size and the member offsets the C compiler gives include/rsvio_gpu.h's (a small program prints
them), and the new entry points are declared, bound and exported."""
import ctypes as C
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
INCLUDE = ROOT / "include"

STRUCTS = {
    "rsvio_ransac_cfg": ("RansacCfg", ["n_hyp", "min_inliers", "seed", "inlier_sq_error", "min_depth"]),
    "rsvio_robust_motion_result": ("RobustMotionResult", ["motion", "ransac_status", "n_pairs", "n_valid_pairs",
                                                           "n_valid_hyp", "best_hyp", "best_count", "n_inliers",
                                                           "reserved", "device_ms"]),
}


def _c_layout(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rsvio_gpu.h"', "int main(void) {"]
    for name, (_, members) in STRUCTS.items():
        lines.append(f'  printf("{name} sizeof %zu\\n", sizeof({name}));')
        for m in members:
            lines.append(f'  printf("{name} {m} %zu\\n", offsetof({name}, {m}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", str(INCLUDE), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    lay = {}
    for line in out.splitlines():
        s, m, v = line.split()
        lay[(s, m)] = int(v)
    return lay


def test_new_structs_match_the_header(tmp_path):
    from rsvio import _lib
    lay = _c_layout(tmp_path)
    for name, (py, members) in STRUCTS.items():
        T = getattr(_lib, py)
        assert C.sizeof(T) == lay[(name, "sizeof")], name
        assert [f[0] for f in T._fields_] == members
        for m in members:
            assert getattr(T, m).offset == lay[(name, m)], (name, m)
    assert lay[("rsvio_ransac_cfg", "sizeof")] == 32
    assert lay[("rsvio_robust_motion_result", "sizeof")] == 224
    assert C.sizeof(_lib.RobustMotionResult) == C.sizeof(_lib.MotionResult) + 40


def test_status_values_match_the_header():
    from rsvio import motion
    text = (INCLUDE / "rsvio_gpu.h").read_text()
    vals = {k: int(v) for k, v in re.findall(r"RSVIO_RANSAC_(\w+)\s*=\s*(-?\d+)", text)}
    assert vals == {"OK": motion.RANSAC_OK, "TOO_FEW_PAIRS": motion.RANSAC_TOO_FEW_PAIRS,
                    "NO_CONSENSUS": motion.RANSAC_NO_CONSENSUS}


def test_entry_points_are_bound_exported_and_validate_before_any_device_call():
    from rsvio import _lib
    lib = _lib.load()
    for s in ("rsvio_track_motion_robust", "rsvio_track_motion_robust_tracker"):
        assert s in _lib.SIG and getattr(lib, s) is not None
    r = _lib.RobustMotionResult()
    assert lib.rsvio_track_motion_robust(None, None, None, 0, None, None, 0, None, None, None, None, None, None, None,
                                         None, None, C.byref(r)) == -1
    assert lib.rsvio_track_motion_robust_tracker(None, None, None, None, None, None, None, None, None, None, None,
                                                 C.byref(r)) == -1


def test_ransac_config_defaults():
    from rsvio.motion import RansacConfig
    c = RansacConfig()
    assert (c.n_hyp, c.min_inliers, c.seed, c.inlier_sq_error, c.min_depth) == (256, 10, 0, 1e-4, 0.1)
    s = RansacConfig(seed=2 ** 64 - 1).to_c()
    assert s.seed == 2 ** 64 - 1 and s.n_hyp == 256
