"""The batched keyframe step's C ABI without a device: the slot structures of rsvio/_lib.py have the
size and the member offsets the C compiler gives include/rsvio_gpu.h's (a small program prints
them), the four entry points are declared, bound and exported, and the argument checks that need no
device answer before any device call and write nothing."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
INCLUDE = ROOT / "include"

LM_MEMBERS = ["lm_mask", "gate", "p_W_out", "info_out", "n_lm", "n_ok", "status", "reserved"]
COV_MEMBERS = ["cov_cc", "cov_pose", "lm_idx", "cov_lm", "lm_flags", "n_sel", "reserved", "info"]
SYMBOLS = ["rsvio_ba_batch_run_active", "rsvio_ba_batch_triangulate", "rsvio_ba_batch_check_landmarks",
           "rsvio_ba_batch_covariance"]


def _c_layout(tmp_path, struct, members):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rsvio_gpu.h"', "int main(void) {",
             f'  printf("sizeof %zu\\n", sizeof({struct}));']
    lines += [f'  printf("{m} %zu\\n", offsetof({struct}, {m}));' for m in members]
    lines += ["  return 0;", "}"]
    src = tmp_path / f"{struct}.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / struct
    subprocess.run(["cc", "-std=c99", "-I", str(INCLUDE), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


@pytest.mark.parametrize("struct,cls,members,size", [
    ("rsvio_ba_landmark_slot", "BaLandmarkSlot", LM_MEMBERS, 48),
    ("rsvio_ba_cov_slot", "BaCovSlot", COV_MEMBERS, 80)])
def test_slots_match_the_header(tmp_path, struct, cls, members, size):
    from rsvio import _lib
    lay = _c_layout(tmp_path, struct, members)
    T = getattr(_lib, cls)
    assert [f[0] for f in T._fields_] == members
    assert C.sizeof(T) == lay["sizeof"] == size
    for m in members:
        assert getattr(T, m).offset == lay[m], m


def test_symbols_are_declared_bound_and_exported():
    from rsvio import _lib
    lib = _lib.load()
    text = (INCLUDE / "rsvio_gpu.h").read_text()
    for s in SYMBOLS:
        assert s in _lib.SIG
        fn = getattr(lib, s)
        assert fn.argtypes == _lib.SIG[s][1] and fn.restype is C.c_int
        assert f" {s}(" in text


def test_null_arguments_are_refused_before_any_device_call():
    """A NULL batch with everything else valid, and (the batch pointer being checked first, no
    handle exists without a device) a NULL slots / cfg / gate beside it: -1, nothing written."""
    from rsvio import _lib
    from rsvio.ba import landmark_gate, lm_cfg
    lib = _lib.load()
    cfg, gate = lm_cfg(), landmark_gate()
    on = (C.c_uint8 * 1)(1)
    res = (_lib.BaResult * 1)()
    C.memset(res, 0x5a, C.sizeof(res))
    lms = (_lib.BaLandmarkSlot * 1)()
    covs = (_lib.BaCovSlot * 1)()
    lms[0].n_ok, lms[0].status, covs[0].info.status = -77, -77, -77
    ms = C.c_double(-3.0)
    before = bytes(res), bytes(lms), bytes(covs)
    for cfg_p, res_p in ((C.byref(cfg), res), (None, res), (C.byref(cfg), None)):
        assert lib.rsvio_ba_batch_run_active(None, on, cfg_p, res_p) == -1
    for fn in (lib.rsvio_ba_batch_triangulate, lib.rsvio_ba_batch_check_landmarks):
        for gate_p, slots_p in ((C.byref(gate), lms), (None, lms), (C.byref(gate), None)):
            assert fn(None, on, gate_p, slots_p, C.byref(ms)) == -1
        assert b"null" in lib.rsvio_last_error()
    for slots_p in (covs, None):
        assert lib.rsvio_ba_batch_covariance(None, on, 2.0, slots_p, C.byref(ms)) == -1
    assert (bytes(res), bytes(lms), bytes(covs)) == before and ms.value == -3.0


def test_python_surface():
    import inspect

    from rsvio.ba import BundleBatch, WindowBatch
    assert list(inspect.signature(BundleBatch.run).parameters) == ["self", "cfg", "active"]
    assert list(inspect.signature(BundleBatch.triangulate).parameters) == ["self", "masks", "gates", "want", "active"]
    assert list(inspect.signature(BundleBatch.check_landmarks).parameters) == ["self", "gates", "active"]
    assert list(inspect.signature(BundleBatch.covariance).parameters) == ["self", "landmarks", "full", "huber_delta",
                                                                         "active"]
    assert list(inspect.signature(WindowBatch.optimize).parameters) == ["self", "cfg", "active"]
