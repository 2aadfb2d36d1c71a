"""bench.py's host-placement helpers on the CPU: the NUMA node's CPU list parsing and the
main-thread pinning switch (the GPU-side effect is measured in profiles/r06z2_pin_cpu_ab.txt and
r06z3_numa_local_ab.txt), and the --dump-outputs writer."""
import bench


def test_parse_cpulist():
    assert bench.parse_cpulist("0-3,8,10-11\n") == {0, 1, 2, 3, 8, 10, 11}
    assert bench.parse_cpulist("64-127,192-255") == set(range(64, 128)) | set(range(192, 256))
    assert bench.parse_cpulist("") == set()


def test_pin_off_is_a_no_op():
    assert bench.pin_main_thread("off") == "off"
    assert bench.pin_main_thread("") == "off"


def test_dump_outputs_writes_float_arrays(tmp_path):
    """--dump-outputs: one float32 / float64 .npy per output of the step; feature rows whose
    valid flag is 0 carry no result and are written as 0."""
    import numpy as np

    class Pinned:  # stands in for the pinned torch tensors of the tracker workload
        def __init__(self, a):
            self.a = a

        def numpy(self):
            return self.a

    class Trk:
        h_valid = Pinned(np.array([[1, 0], [0, 1], [1, 1]], np.uint8))
        h_out = Pinned(np.arange(36, dtype=np.float32).reshape(3, 2, 6) + 1)

    pose, pw = np.full((10, 7), 0.5), np.full((4, 3), 2.0)
    bench.dump_outputs(tmp_path / "d", Trk, (pose, pw), 5)
    got = {p.stem: np.load(p) for p in (tmp_path / "d").glob("*.npy")}
    assert sorted(got) == ["ba_iterations", "ba_landmarks", "ba_poses", "tracker_features", "tracker_valid"]
    assert got["tracker_valid"].dtype == np.float32 and got["tracker_features"].dtype == np.float32
    assert all(got[k].dtype == np.float64 for k in ("ba_poses", "ba_landmarks", "ba_iterations"))
    assert np.array_equal(got["tracker_valid"], [[1, 0], [0, 1], [1, 1]])
    want = Trk.h_out.a.copy()
    want[0, 1] = want[1, 0] = 0
    assert np.array_equal(got["tracker_features"], want)
    assert np.array_equal(got["ba_poses"], pose) and np.array_equal(got["ba_landmarks"], pw)
    assert got["ba_iterations"].tolist() == [5.0]
