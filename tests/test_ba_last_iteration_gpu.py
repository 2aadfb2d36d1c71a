"""The last iteration of a chunk with the state export on (K6's "last of chunk" form, ba.hip).

With the export on, the final K6 of every chunk of LM iterations copies the CURRENT state into
the pinned export buffer and evaluates the trial's cost without linearising it; K7 skips its own
copy when it ends the solve for the buffer that K6 exported, and a solve that goes on past the
chunk runs that iteration's full K6 again first.  None of it may change a result: every solve
below equals, bit for bit (np.array_equal), the same solve on a fresh handle that never turned
the export on (plain kernels, state() copied from the device buffers).

The window is small -- 5 keyframes, 96 landmarks over 4 keyframes each, 768 observations, two
K6 waves -- and the CPU oracle fixes what each configuration must do on it (asserted first by
every test, so none can pass on a trivial case):

    default               status 1 (cost tolerance)   6 iterations
    cost_tolerance=1e-2   status 1                    3
    cost_tolerance=1e-1   status 1                    2
    max_iterations=2      status 3 (max iterations)   2
    landmarks 0-3 without observations (736 left): status 1, 6 iterations, their points unchanged

A handle's first chunk is its previous solve's iteration count (3 on a new handle), which is how
the tests steer the guess.  Tolerances against the oracle are test_ba_gpu.py's: poses 1e-7,
points 1e-6.
"""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFGS = {
    "default": {},
    "tol1e-2": {"cost_tolerance": 1e-2},
    "tol1e-1": {"cost_tolerance": 1e-1},
    "max2": {"max_iterations": 2},
    "max1": {"max_iterations": 1},
    "max3": {"max_iterations": 3},
}
ORACLE = {"default": (1, 6), "tol1e-2": (1, 3), "tol1e-1": (1, 2), "max2": (3, 2)}  # (status, iterations)


def _window(seed, init_seed, **kw):
    from rsvio import synthetic as S
    return S.ba_problem(n_kf=5, n_lm=96, kf_per_lm=4, seed=seed, init_seed=init_seed, **kw)


def _handle(prob):
    from rsvio.ba import BundleAdjuster
    ba = BundleAdjuster(max_keyframes=21, max_landmarks=prob.n_lm, max_observations=prob.n_obs)
    ba.set_problem_from(prob)
    return ba


def _exporting(prob):
    """A handle with the window set and the export turned on (by a first state() call)."""
    ba = _handle(prob)
    p0, w0 = ba.state()
    assert np.array_equal(p0, prob.pose7) and np.array_equal(w0, prob.p_W)
    return ba


def _solve(ba, name="default", use_async=False):
    from rsvio.ba import lm_cfg
    cfg = lm_cfg(**CFGS[name])
    if use_async:
        ba.run_async(cfg)
        r = ba.wait()
    else:
        r = ba.run(cfg)
    pose, pw = ba.state()
    return (r.status, r.iterations, r.final_cost), pose.copy(), pw.copy()


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


class _Refs:
    """Per (window, configuration), computed once and never modified: the solve on a fresh handle
    without the export (device copy), and the oracle's."""

    def __init__(self, gpu, oracle):
        self.oracle = oracle
        self.win = _window(33, 34)
        self.alt = _window(35, 36, depth_noise=0.2)  # (the oracle needs 7 iterations on this one)
        keep = self.win.obs_lm >= 4
        self.bare = dataclasses.replace(self.win, obs_lm=self.win.obs_lm[keep], obs_kf=self.win.obs_kf[keep],
                                        obs_cam=self.win.obs_cam[keep], obs_uv=self.win.obs_uv[keep])
        self._fresh, self._orc = {}, {}

    def fresh(self, prob, name="default"):
        key = (id(prob), name)
        if key not in self._fresh:
            ba = _handle(prob)
            out = _solve(ba, name)
            ba.close()
            for a in out[1:]:
                a.setflags(write=False)
            self._fresh[key] = out
        return self._fresh[key]

    def orc(self, prob, name="default"):
        key = (id(prob), name)
        if key not in self._orc:
            po, pwo, ro = self.oracle.ba_solve(prob, self.oracle.lm_cfg(**CFGS[name]))
            self._orc[key] = ((ro.status, ro.iterations), po, pwo)
        return self._orc[key]

    def precondition(self, *names):
        assert self.win.n_obs == 768
        for n in names:
            assert self.orc(self.win, n)[0] == ORACLE[n], n


@pytest.fixture(scope="module")
def refs(gpu, oracle):
    return _Refs(gpu, oracle)


def test_right_guess_descriptor_and_by_value(gpu, refs):
    """The chunk is as long as the solve (6): its last K6 exports the state and K7 only stamps."""
    refs.precondition("default")
    want = refs.fresh(refs.win)
    assert want[0][:2] == ORACLE["default"]
    ba = _exporting(refs.win)
    assert _same(_solve(ba), want)           # (first chunk 3: leaves the guess at 6)
    got = _solve(ba)                          # re-solve: by-value graph, first chunk 6
    assert got[0][:2] == ORACLE["default"] and _same(got, want)
    ba.set_problem_from(refs.win)             # a newly set window: descriptor graph, first chunk 6
    got = _solve(ba)
    assert got[0][:2] == ORACLE["default"] and _same(got, want)
    got = _solve(ba, use_async=True)          # and once more by value, through run_async / wait
    assert _same(got, want)
    ba.close()


def test_guess_too_short_redoes_last_k6(gpu, refs):
    """A first chunk shorter than the solve: its cost-only K6 is run again in full before the next
    chunk, in the descriptor graph (a new handle guesses 3) and in the by-value one (guess 2, then
    chunks of 2, each ending in a cost-only K6)."""
    refs.precondition("default", "tol1e-1")
    want = refs.fresh(refs.win)
    assert want[0][:2] == ORACLE["default"]
    ba = _exporting(refs.win)
    assert _same(_solve(ba), want)            # descriptor graph, chunks 3 + 2 + 2
    short = _solve(ba, "tol1e-1")
    assert short[0][:2] == ORACLE["tol1e-1"] and _same(short, refs.fresh(refs.win, "tol1e-1"))
    assert _same(_solve(ba), want)            # by-value graph, chunks 2 + 2 + 2
    ba.close()


def test_guess_too_long_k7_copies(gpu, refs):
    """Convergence inside the chunk: the solve ends before the chunk's last K6."""
    refs.precondition("default", "tol1e-1", "tol1e-2")
    ba = _exporting(refs.win)
    _solve(ba)
    assert _solve(ba)[0][:2] == ORACLE["default"]   # the guess is 6 now
    for name in ("tol1e-1", "tol1e-2"):
        _solve(ba)                                   # back to a guess of 6
        got = _solve(ba, name)
        assert got[0][:2] == ORACLE[name]
        assert _same(got, refs.fresh(refs.win, name))
    ba.close()


def test_max_iterations_applies_last_step(gpu, refs):
    """max_iterations=2 ends on an accepted step: cur flipped after K6's export, K7 copies."""
    refs.precondition("max2")
    want = refs.fresh(refs.win, "max2")
    (so, pose_o, pw_o) = refs.orc(refs.win, "max2")
    assert want[0][:2] == ORACLE["max2"] == so
    ba = _exporting(refs.win)
    for _ in range(2):  # descriptor graph, then by value
        got = _solve(ba, "max2")
        assert got[0][:2] == ORACLE["max2"] and _same(got, want)
        assert np.abs(got[1] - pose_o).max() < 1e-7 and np.abs(got[2] - pw_o).max() < 1e-6
        assert not np.array_equal(got[2], refs.win.p_W)  # (a step was applied)
    ba.close()


@pytest.mark.parametrize("name", ["max1", "max2", "max3"])
def test_cost_only_trial_cost_is_bit_identical(gpu, refs, name):
    """A solve cut off by max_iterations on an accepted step reports that step's trial cost as its
    final cost: here the cost-only K6 computed it, on the fresh handle the linearising K6 did."""
    refs.precondition("default")
    want = refs.fresh(refs.win, name)
    n = CFGS[name]["max_iterations"]
    assert want[0][:2] == (3, n) == refs.orc(refs.win, name)[0]
    prev = refs.fresh(refs.win, "max%d" % (n - 1))[0][2] if n > 1 else None
    assert want[0][2] != prev                  # (the last step was accepted: the cost moved)
    ba = _exporting(refs.win)
    for _ in range(2):  # descriptor graph, then by value
        assert _same(_solve(ba, name), want)
    ba.close()


def test_landmarks_without_observations(gpu, refs):
    """Landmarks 0-3 have no slot in any K6 wave: the export still returns their initial points."""
    refs.precondition("default")
    bare = refs.bare
    assert bare.n_obs == 736
    (so, pose_o, pw_o) = refs.orc(bare)
    assert so == (1, 6) and np.array_equal(pw_o[:4], bare.p_W[:4])
    want = refs.fresh(bare)
    ba = _exporting(bare)
    for _ in range(3):  # guess 3 (too short), then 6 by value; the last K6 exports from the second on
        got = _solve(ba)
        assert got[0][:2] == so and _same(got, want)
        assert np.array_equal(got[2][:4], bare.p_W[:4])
        assert np.abs(got[1] - pose_o).max() < 1e-7 and np.abs(got[2] - pw_o).max() < 1e-6
    ba.close()


def test_window_alternation_never_serves_a_stale_export(gpu, refs):
    """Two windows alternating on one handle, as the protocol step does.  They differ in their
    iteration counts (6 and 7), so every round's guess is the other window's: one too long (the
    descriptor graph replayed with a longer chunk), one too short."""
    refs.precondition("default")
    wins = (refs.win, refs.alt)
    assert refs.orc(refs.alt)[0] == (1, 7)
    for w in wins:
        assert refs.fresh(w)[0][:2] == refs.orc(w)[0]
    assert not np.array_equal(refs.fresh(wins[0])[2], refs.fresh(wins[1])[2])
    ba = _exporting(refs.win)
    for rnd in range(10):
        w = wins[rnd & 1]
        ba.set_problem_from(w)
        got = _solve(ba, use_async=True)
        assert _same(got, refs.fresh(w)), rnd
    ba.close()
