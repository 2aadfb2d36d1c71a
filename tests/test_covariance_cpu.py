"""CPU side of rsvio_ba_covariance: the yardstick of tests/test_covariance_gpu.py pinned (its two
reference routes agree with each other), and the ABI (header, ctypes binding)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import covariance_reference as R

ROOT = Path(__file__).resolve().parent.parent


def _problem(name):
    from rsvio import synthetic as S
    if name == "staircase":
        return S.ba_pattern_problem("staircase", 20)
    n_kf, n_lm = name
    return S.ba_problem(n_kf, n_lm, kf_per_lm=min(6, n_kf))


@pytest.mark.parametrize("case", [(3, 40), (11, 200), "staircase"], ids=str)
def test_reference_routes_agree(oracle, case):
    """inv(S) of the oracle's reduced system and the blocks of inv(H) of the numpy-assembled
    Hessian agree within 1e-10 scaled (measured: 7e-12 at most over these cases), and every
    landmark block of inv(H) is positive definite."""
    prob = _problem(case)
    a = R.schur_pose_cov(oracle, prob)
    b, lm, observed = R.dense_cov(oracle, prob)
    print(f"{case}: pose routes differ by {R.scaled_err(a, b):.3g} scaled, cond(S) {np.linalg.cond(np.linalg.inv(a)):.3g}")
    assert a.shape == b.shape
    assert R.scaled_err(a, b) <= 1e-10
    assert observed.all() and (np.linalg.eigvalsh(lm) > 0).all()


def test_header_and_binding():
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "rsvio_gpu.h").read_text(), flags=re.S)
    m = re.search(r"int\s+rsvio_ba_covariance\s*\(([^;]*)\)\s*;", hdr)
    assert m, "rsvio_ba_covariance is not declared"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    assert "rsvio_cov_info" in hdr
    for name in ("RSVIO_COV_OK = 1", "RSVIO_COV_CAMERA_SINGULAR = -1", "RSVIO_COV_LANDMARK_SINGULAR = -2",
                 "RSVIO_COV_LM_OK = 1", "RSVIO_COV_LM_NOT_OBSERVED = 2"):
        assert name in hdr
    from rsvio import _lib
    res, argtypes = _lib.SIG["rsvio_ba_covariance"]
    assert res is C.c_int and len(argtypes) == n_args == 9
    # four int32 and two doubles: 32 bytes, the C layout of the typedef as declared
    assert C.sizeof(_lib.CovInfo) == 32
    assert [f[0] for f in _lib.CovInfo._fields_] == ["status", "n_free", "n_singular", "reserved", "cost", "device_ms"]


def test_integration_md_carries_the_export():
    text = (ROOT / "INTEGRATION.md").read_text()
    assert "rsvio_ba_covariance" in text and "rsvio_cov_info" in text
