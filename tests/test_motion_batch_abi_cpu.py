"""rsvio_motion_frame and the rsvio_pnp_batch_* entry points without a device: the ctypes structure
of rsvio/_lib.py has the size and the member offsets the C compiler gives include/rsvio_gpu.h's (a
small program prints them), the four symbols are declared, bound and exported, and the argument
checks that need no device answer before any device call."""
import ctypes as C
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
INCLUDE = ROOT / "include"

MEMBERS = ["ids_l", "uv_l", "n_l", "ids_r", "uv_r", "n_r", "T_W_B_last_kf", "T_C_B2", "cfg", "samples", "mask_l",
           "mask_r", "hyp_count", "on_device", "id_stride"]
SYMBOLS = ["rsvio_pnp_batch_create", "rsvio_pnp_batch_track_motion", "rsvio_pnp_batch_track_motion_robust",
           "rsvio_pnp_batch_destroy"]


def _c_layout(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rsvio_gpu.h"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(rsvio_motion_frame));']
    lines += [f'  printf("{m} %zu\\n", offsetof(rsvio_motion_frame, {m}));' for m in MEMBERS]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", str(INCLUDE), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_motion_frame_matches_the_header(tmp_path):
    from rsvio import _lib
    lay = _c_layout(tmp_path)
    T = _lib.MotionFrame
    assert [f[0] for f in T._fields_] == MEMBERS
    assert C.sizeof(T) == lay["sizeof"] == 112
    for m in MEMBERS:
        assert getattr(T, m).offset == lay[m], m


def test_symbols_are_declared_bound_and_exported():
    from rsvio import _lib
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in _lib.SIG
        fn = getattr(lib, s)
        assert fn.argtypes == _lib.SIG[s][1]
    text = (INCLUDE / "rsvio_gpu.h").read_text()
    for s in SYMBOLS:
        assert f" {s}(" in text


def test_create_validates_before_any_device_call():
    from rsvio import _lib
    lib = _lib.load()
    out = C.c_void_p()
    one = (C.c_void_p * 1)(None)
    many = (C.c_void_p * 4097)()
    assert lib.rsvio_pnp_batch_create(None, 1, C.byref(out)) == -1
    assert lib.rsvio_pnp_batch_create(one, 0, C.byref(out)) == -1
    assert lib.rsvio_pnp_batch_create(many, 4097, C.byref(out)) == -1
    assert lib.rsvio_pnp_batch_create(one, -1, C.byref(out)) == -1
    assert lib.rsvio_pnp_batch_create(one, 1, None) == -1
    assert lib.rsvio_pnp_batch_create(one, 1, C.byref(out)) == -1   # a NULL handle in the list
    assert out.value is None


def test_runs_refuse_a_null_batch():
    from rsvio import _lib
    from rsvio.motion import RansacConfig, pnp_cfg
    lib = _lib.load()
    frames = (_lib.MotionFrame * 1)()
    cfg, rule, rc = pnp_cfg(), _lib.KeyframeRule(0.05, 0.05), RansacConfig().to_c()
    res = (_lib.MotionResult * 1)()
    rres = (_lib.RobustMotionResult * 1)()
    before = bytes(res), bytes(rres)
    assert lib.rsvio_pnp_batch_track_motion(None, C.addressof(frames), C.byref(cfg), C.byref(rule),
                                            C.addressof(res), None) == -1
    assert lib.rsvio_pnp_batch_track_motion_robust(None, C.addressof(frames), C.byref(cfg), C.byref(rule),
                                                   C.byref(rc), C.addressof(rres), None) == -1
    assert (bytes(res), bytes(rres)) == before
    lib.rsvio_pnp_batch_destroy(None)   # like free(NULL)


def test_motion_frame_dataclass_fields():
    import dataclasses

    from rsvio.motion import MotionBatch, MotionFrame
    names = [f.name for f in dataclasses.fields(MotionFrame)]
    assert names[:8] == ["ids_l", "uv_l", "ids_r", "uv_r", "T_W_B_last_kf", "T_C_B2", "cfg", "samples"]
    f = MotionFrame(None, None, None, None, None, None)
    assert f.cfg is None and f.samples is None and not f.on_device and f.id_stride == 0
    for m in ("track_motion", "track_motion_robust", "close"):
        assert callable(getattr(MotionBatch, m))
