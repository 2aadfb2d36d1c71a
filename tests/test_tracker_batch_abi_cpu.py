"""rsvio_stereo_frame, the rsvio_tracker_batch_* entry points and rsvio_tracker_device_lists without
a device: the ctypes structure of rsvio/_lib.py has the size and the member offsets the C compiler
gives include/rsvio_gpu.h's (a small program prints them), the four symbols are declared, bound and
exported, and the argument checks that need no device answer before any device call."""
import ctypes as C
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
INCLUDE = ROOT / "include"

MEMBERS = ["left", "right", "stride", "out_l", "cap_l", "out_r", "cap_r", "n_l", "n_r", "on_device", "status"]
SYMBOLS = ["rsvio_tracker_batch_create", "rsvio_tracker_batch_process_frames", "rsvio_tracker_batch_destroy",
           "rsvio_tracker_device_lists"]


def _c_layout(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rsvio_gpu.h"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(rsvio_stereo_frame));',
             '  printf("feature %zu\\n", sizeof(rsvio_feature));']
    lines += [f'  printf("{m} %zu\\n", offsetof(rsvio_stereo_frame, {m}));' for m in MEMBERS]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", str(INCLUDE), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_stereo_frame_matches_the_header(tmp_path):
    from rsvio import _lib
    from rsvio.tracker import FEATURE_DTYPE
    lay = _c_layout(tmp_path)
    T = _lib.StereoFrame
    assert [f[0] for f in T._fields_] == MEMBERS
    assert C.sizeof(T) == lay["sizeof"] == 80
    for m in MEMBERS:
        assert getattr(T, m).offset == lay[m], m
    assert FEATURE_DTYPE.itemsize == C.sizeof(_lib.Feature) == lay["feature"] == 32   # id_stride of a device list


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
    many = (C.c_void_p * 1025)()
    assert lib.rsvio_tracker_batch_create(None, 1, C.byref(out)) == -1
    assert lib.rsvio_tracker_batch_create(one, 0, C.byref(out)) == -1
    assert lib.rsvio_tracker_batch_create(one, -1, C.byref(out)) == -1
    assert lib.rsvio_tracker_batch_create(many, 1025, C.byref(out)) == -1
    assert lib.rsvio_tracker_batch_create(one, 1, None) == -1
    assert lib.rsvio_tracker_batch_create(one, 1, C.byref(out)) == -1   # a NULL handle in the list
    assert b"slot 0" in lib.rsvio_last_error()
    assert out.value is None


def test_process_frames_refuses_a_null_batch_and_writes_nothing():
    from rsvio import _lib
    lib = _lib.load()
    frames = (_lib.StereoFrame * 1)()
    C.memset(C.addressof(frames), 0xA5, C.sizeof(frames))
    ms = C.c_double(-7.0)
    assert lib.rsvio_tracker_batch_process_frames(None, C.addressof(frames), C.byref(ms)) == -1
    assert bytes(frames) == b"\xa5" * C.sizeof(frames) and ms.value == -7.0
    lib.rsvio_tracker_batch_destroy(None)   # like free(NULL)


def test_device_lists_refuses_null_arguments():
    from rsvio import _lib
    lib = _lib.load()
    p, n = C.c_void_p(), C.c_size_t(5)
    assert lib.rsvio_tracker_device_lists(None, C.byref(p), C.byref(n), C.byref(p), C.byref(n), None, None) == -1
    assert p.value is None and n.value == 5


def test_python_surface():
    from rsvio import StereoPatchTracker, TrackerBatch
    for m in ("process_frames", "close"):
        assert callable(getattr(TrackerBatch, m))
    assert callable(StereoPatchTracker.device_lists)
