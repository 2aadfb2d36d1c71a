"""The CPU reference of motion-predicted tracking (tests/seeded_tracking_reference.py) and its fixture
(rsvio.synthetic.rotating_scene_pair), without a device.  These are conditions on the reference and
the fixture, not on the code under test: the reference collapses to the oracle's track_points when
every seed is the feature's own position, and the fixture shows what the feature is for -- at a yaw
of 8 degrees the unseeded tracker loses almost every track and the seeded one keeps them."""
import numpy as np

import seeded_tracking_reference as ref
from seeded_tracking_reference import H, LEVELS, W


def test_seed_at_position_is_the_oracle_bit_for_bit(oracle):
    pyr0, pyr1, aff, _, _, _ = ref.fixture(0.5)
    assert len(aff) == 96
    want, want_valid = oracle.track_points(pyr0, pyr1, W, H, LEVELS, aff)
    got, got_valid = ref.track_points_seeded(pyr0, pyr1, W, H, LEVELS, aff, aff[:, 4:6])
    assert np.array_equal(got_valid, want_valid)
    assert got.tobytes() == want.tobytes()
    assert 80 <= int(want_valid.sum()) < 96   # both outcomes are compared


def test_fixture_at_8_degrees_needs_the_seeds(oracle):
    """Measured with the oracle on this fixture: the unseeded tracker keeps 5 of the 96 features, the
    seeded reference 86; 88 of the 96 seeds are inside the image."""
    pyr0, pyr1, aff, cam, R, _ = ref.fixture(8.0)
    assert len(aff) == 96
    _, unseeded = oracle.track_points(pyr0, pyr1, W, H, LEVELS, aff)
    seeds, seeded = ref.predict_seeds(cam, R, aff[:, 4:6], W, H)
    out, valid = ref.track_points_seeded(pyr0, pyr1, W, H, LEVELS, aff, seeds)
    print("unseeded keeps", int(unseeded.sum()), "seeded keeps", int(valid.sum()), "seeds inside", int(seeded.sum()))
    assert int(unseeded.sum()) <= 15
    assert int(valid.sum()) >= 80
    # the results sit at the seeds: the hint is exact for a rotation about the camera centre
    d = np.linalg.norm(out[valid, 4:6] - seeds[valid], axis=1)
    assert np.median(d) < 0.5


def test_fallback_is_exercised_at_8_degrees():
    _, _, aff, cam, R, _ = ref.fixture(8.0)
    seeds, seeded = ref.predict_seeds(cam, R, aff[:, 4:6], W, H)
    assert int(seeded.sum()) == 88 and len(seeded) == 96
    assert np.array_equal(seeds[~seeded], aff[~seeded, 4:6])          # the fallback: the own position
    inside = (seeds[:, 0] >= 0) & (seeds[:, 0] <= W - 1) & (seeds[:, 1] >= 0) & (seeds[:, 1] <= H - 1)
    assert inside.all()
    # the identity hint seeds every feature at (very nearly) its own pixel
    s0, ok0 = ref.predict_seeds(cam, np.eye(3), aff[:, 4:6], W, H)
    assert ok0.all() and np.abs(s0 - aff[:, 4:6]).max() < 1e-3
