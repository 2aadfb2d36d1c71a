"""rsvio_motion_cov_info and the three motion covariance entry points without a device: the ctypes
structure of rsvio/_lib.py has the size and the member offsets the C compiler gives
include/rsvio_gpu.h's (a small program prints them), the symbols are declared, bound and exported
with their argument counts, and the argument checks that need no device answer before any device
call and write nothing."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
INCLUDE = ROOT / "include"

MEMBERS = ["status", "n_observations", "n_downweighted", "reserved", "cost", "min_pivot", "kernel_ms"]
SYMBOLS = {"rsvio_motion_covariance": 14, "rsvio_motion_covariance_tracker": 9, "rsvio_pnp_batch_covariance": 7}


def _c_layout(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rsvio_gpu.h"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(rsvio_motion_cov_info));',
             '  printf("OK %d\\n", (int)RSVIO_MCOV_OK);', '  printf("TOO_FEW %d\\n", (int)RSVIO_MCOV_TOO_FEW);',
             '  printf("SINGULAR %d\\n", (int)RSVIO_MCOV_SINGULAR);',
             '  printf("frame %zu\\n", sizeof(rsvio_motion_frame));']
    lines += [f'  printf("{m} %zu\\n", offsetof(rsvio_motion_cov_info, {m}));' for m in MEMBERS]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", str(INCLUDE), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_cov_info_matches_the_header(tmp_path):
    from rsvio import _lib, motion
    lay = _c_layout(tmp_path)
    T = _lib.MotionCovInfo
    assert [f[0] for f in T._fields_] == MEMBERS
    assert C.sizeof(T) == lay["sizeof"] == 40
    for m in MEMBERS:
        assert getattr(T, m).offset == lay[m], m
    assert (lay["OK"], lay["TOO_FEW"], lay["SINGULAR"]) == (1, -1, -2)
    assert (motion.MCOV_OK, motion.MCOV_TOO_FEW, motion.MCOV_SINGULAR) == (1, -1, -2)
    assert lay["frame"] == C.sizeof(_lib.MotionFrame) == 112     # rsvio_motion_frame keeps its layout


def test_symbols_are_declared_bound_and_exported():
    from rsvio import _lib
    lib = _lib.load()
    text = (INCLUDE / "rsvio_gpu.h").read_text()
    for s, n_args in SYMBOLS.items():
        assert s in _lib.SIG
        assert len(_lib.SIG[s][1]) == n_args
        fn = getattr(lib, s)
        assert fn.argtypes == _lib.SIG[s][1] and fn.restype is C.c_int
        assert f" {s}(" in text


def _buffers():
    cov = np.full(36, 7.0)
    info = (C.c_uint8 * 40)(*([0xAB] * 40))
    return cov, info


def test_single_calls_refuse_bad_arguments_before_any_device_call():
    from rsvio import _lib
    lib = _lib.load()
    T = np.eye(4).reshape(16)
    tcb = np.tile(np.eye(4).reshape(16), 2)
    ids = np.arange(4, dtype=np.uint64)
    uv = np.zeros((4, 2), np.float32)
    cov, info = _buffers()
    before = cov.copy(), bytes(info)
    fake = C.c_void_p(8)    # never dereferenced: every check below fails first

    def single(h, ids_l, uv_l, n_l, T_, tcb_, delta, cov_, info_):
        return lib.rsvio_motion_covariance(h, ids_l, uv_l, n_l, None, None, 0, None, None, T_, tcb_, C.c_double(delta),
                                           cov_, info_)

    p = _lib.ptr
    ip = C.cast(info, C.POINTER(_lib.MotionCovInfo))
    assert single(None, p(ids), p(uv), 4, p(T), p(tcb), 2.0, p(cov), ip) == -1           # no handle
    assert single(fake, None, p(uv), 4, p(T), p(tcb), 2.0, p(cov), ip) == -1             # n_l without ids
    assert single(fake, p(ids), None, 4, p(T), p(tcb), 2.0, p(cov), ip) == -1
    assert single(fake, p(ids), p(uv), 4, None, p(tcb), 2.0, p(cov), ip) == -1           # no pose
    assert single(fake, p(ids), p(uv), 4, p(T), None, 2.0, p(cov), ip) == -1
    assert single(fake, p(ids), p(uv), 4, p(T), p(tcb), 2.0, None, ip) == -1
    assert single(fake, p(ids), p(uv), 4, p(T), p(tcb), 2.0, p(cov), None) == -1
    for delta in (0.0, -1.0, float("nan")):
        assert single(fake, p(ids), p(uv), 4, p(T), p(tcb), delta, p(cov), ip) == -1
    assert single(fake, p(ids), p(uv), 4097, p(T), p(tcb), 2.0, p(cov), ip) == -4        # RSVIO_ERR_CAPACITY
    assert b"4096" in lib.rsvio_last_error()
    tr = lib.rsvio_motion_covariance_tracker
    assert tr(None, fake, None, None, p(T), p(tcb), C.c_double(2.0), p(cov), ip) == -1
    assert tr(fake, None, None, None, p(T), p(tcb), C.c_double(2.0), p(cov), ip) == -1
    assert tr(fake, fake, None, None, None, p(tcb), C.c_double(2.0), p(cov), ip) == -1
    assert tr(fake, fake, None, None, p(T), p(tcb), C.c_double(0.0), p(cov), ip) == -1
    assert tr(fake, fake, None, None, p(T), p(tcb), C.c_double(2.0), None, ip) == -1
    assert np.array_equal(cov, before[0]) and bytes(info) == before[1]


def test_batch_call_refuses_bad_arguments_before_any_device_call():
    from rsvio import _lib
    lib = _lib.load()
    frames = (_lib.MotionFrame * 1)()
    T = np.eye(4).reshape(1, 16)
    cov, info = _buffers()
    before = cov.copy(), bytes(info)
    fake = C.c_void_p(8)
    p = _lib.ptr
    ip = C.cast(info, C.POINTER(_lib.MotionCovInfo))
    f = lib.rsvio_pnp_batch_covariance
    assert f(None, C.addressof(frames), p(T), C.c_double(2.0), p(cov), ip, None) == -1
    assert f(fake, None, p(T), C.c_double(2.0), p(cov), ip, None) == -1
    assert f(fake, C.addressof(frames), None, C.c_double(2.0), p(cov), ip, None) == -1
    assert f(fake, C.addressof(frames), p(T), C.c_double(2.0), None, ip, None) == -1
    assert f(fake, C.addressof(frames), p(T), C.c_double(2.0), p(cov), None, None) == -1
    for delta in (0.0, float("nan")):
        assert f(fake, C.addressof(frames), p(T), C.c_double(delta), p(cov), ip, None) == -1
    assert np.array_equal(cov, before[0]) and bytes(info) == before[1]


def test_python_surface():
    import dataclasses

    import rsvio
    from rsvio.estimator import Estimator, FrameResult
    from rsvio.motion import MotionBatch, MotionTracker, PoseCovariance
    assert rsvio.PoseCovariance is PoseCovariance and "PoseCovariance" in rsvio.__all__
    assert [f.name for f in dataclasses.fields(PoseCovariance)] == [
        "status", "cov", "n_observations", "n_downweighted", "cost", "min_pivot", "kernel_ms"]
    for m in ("covariance", "covariance_tracker"):
        assert callable(getattr(MotionTracker, m))
    assert callable(MotionBatch.covariance)
    fields = {f.name: f for f in dataclasses.fields(FrameResult)}
    assert fields["pose_covariance"].default is None
    import inspect
    assert inspect.signature(Estimator.__init__).parameters["pose_covariance"].default is False
    sig = inspect.signature(MotionTracker.covariance).parameters
    assert sig["huber_delta"].default == 2.0 and sig["mask_l"].default is None and sig["mask_r"].default is None
