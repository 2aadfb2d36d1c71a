"""The BA's free-keyframe dispatch (rs-vio_amd/csrc/ba_dispatch.hpp) on the CPU.

Every camera-solve launch site of ba.hip picks its kernel template through dispatch_panel_nf
(1..10 free keyframes) or dispatch_block_nf (13, 16, 20: the sizes bk_template_nf pads to).
tools/ba_dispatch_check.cpp compiles the header with g++ alone -- it includes nothing of HIP -- and
prints what each nf in 0..24 reached: a wrong constant would launch a kernel built for another
system size, a miss that calls f anyway would launch one where the site reports an error.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANEL = set(range(1, 11))
BLOCK = {13, 16, 20}


@pytest.fixture(scope="module")
def reached(tmp_path_factory):
    """{(which, nf): (returned, calls of f, the constant f got or -1)} for nf in 0..24"""
    if shutil.which("g++") is None:
        pytest.skip("g++ absent")
    out = str(tmp_path_factory.mktemp("dispatch") / "ba_dispatch_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rs-vio_amd", "csrc"),
                    os.path.join(ROOT, "tools", "ba_dispatch_check.cpp"), "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split() for ln in r.stdout.strip().splitlines()]
    got = {(w, int(nf)): (int(hit), int(calls), int(c)) for w, nf, hit, calls, c in rows}
    assert len(got) == 50
    return got


def test_panel_sizes_reach_their_own_constant(reached):
    for nf in range(1, 11):
        assert reached["panel", nf] == (1, 1, nf)


def test_block_sizes_reach_their_own_constant(reached):
    for nf in (13, 16, 20):
        assert reached["block", nf] == (1, 1, nf)


def test_a_miss_returns_false_without_calling(reached):
    for nf in (0, 11, 21):
        assert reached["panel", nf] == (0, 0, -1)
        assert reached["block", nf] == (0, 0, -1)
    for nf in range(25):
        if nf not in PANEL:
            assert reached["panel", nf] == (0, 0, -1)
        if nf not in BLOCK:
            assert reached["block", nf] == (0, 0, -1)
