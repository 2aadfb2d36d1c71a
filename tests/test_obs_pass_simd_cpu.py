"""set_problem's vectorised key + mask sweep (rs-vio_amd/csrc/obs_pass.hpp) against a plain loop.

tools/obs_pass_equiv.cpp is a stand-alone program: it compares rsvio_obs::observation_pass with a
reference loop of its own (one observation at a time, no SIMD, masks by read-modify-write, duplicates
and landmarks in two runs found by explicit checks) over every vector tail (n_obs 0 .. 17), runs of
every length 1-13 at every offset against the 8-wide groups, landmarks without observations, one
camera only, n_kf 32 (bit 63), n_lm 1, 1,000 random landmark-major windows of up to 600 observations,
every reject (index out of range, duplicate inside a group and across groups, a landmark in two
adjacent or distant runs) planted at every lane position and in the tail, and (u, v) values that are
not f32 or NaN at every position -- at every dispatch level the host supports, the scalar one
included: equal return value, and equal key[], m2[], uv32[] and *narrowed when that value is true.

It is built twice: plainly, and with -fsanitize=address,undefined (a stand-alone binary, nothing
preloaded), which checks the unaligned loads and the tails against reads past the arrays' ends.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "obs_pass_equiv.cpp")
INC = os.path.join(ROOT, "rs-vio_amd", "csrc")


def _build(out, flags):
    subprocess.run(["g++", "-std=c++17", "-pthread", *flags, "-I", INC, SRC, "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def equiv_bin(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("obs_equiv") / "obs_pass_equiv"), ["-O2"])


@pytest.fixture(scope="module")
def equiv_san_bin(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("obs_equiv_san") / "obs_pass_equiv_san"),
                  ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                   "-static-libasan", "-static-libubsan"])  # (the runtimes inside the binary)


def _env():
    env = dict(os.environ)
    env.pop("RSVIO_OBS_SIMD", None)  # the program sets the level itself
    env.pop("RSVIO_BA_HOST_THREADS", None)
    return env


def _levels(binary):
    r = subprocess.run([binary, "--levels"], env=_env(), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    levels = r.stdout.split()
    assert levels and levels[0] == "scalar" and set(levels) <= {"scalar", "avx2", "avx512"}
    return levels


def _check_report(r, levels):
    assert r.returncode == 0, r.stdout + r.stderr
    seen = {}
    for m in re.finditer(r"level (\w+): (\d+) cases \((\d+) accepted, (\d+) rejected\), (\d+) mismatches", r.stdout):
        seen[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    assert list(seen) == levels, r.stdout
    for cases, accepted, rejected, mismatches in seen.values():
        assert mismatches == 0
        # both outcomes are exercised, at every level alike
        assert cases > 3000 and accepted > 1000 and rejected > 1000
    assert len(set(seen.values())) == 1


def test_every_level_equals_the_reference_loop(equiv_bin):
    levels = _levels(equiv_bin)
    r = subprocess.run([equiv_bin], env=_env(), capture_output=True, text=True, timeout=120)
    _check_report(r, levels)


def test_forced_scalar_level(equiv_bin):
    r = subprocess.run([equiv_bin, "--level", "scalar"], env=_env(), capture_output=True, text=True, timeout=120)
    _check_report(r, ["scalar"])


def test_every_level_under_address_and_ub_sanitizers(equiv_san_bin):
    levels = _levels(equiv_san_bin)
    r = subprocess.run([equiv_san_bin], env=_env(), capture_output=True, text=True, timeout=300)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    _check_report(r, levels)
