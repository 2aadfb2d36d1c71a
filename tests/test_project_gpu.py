"""rsvio_project / rsvio_project_d (the forward projection of both camera models) on the GPU against
oracle.project, bit for bit in f64: radtan (EuRoC, k3 set) and EUCM (TUM-VI, and alpha < 1/2 where
den <= 0 is reachable), n in {0, 1, 1000}, points behind the camera (Z <= 0, the origin) included."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _cams():
    from rsvio.camera import EUROC, TUM_VI, Camera
    k3 = Camera.opencv5(*EUROC[0].params[:8], k3=0.0123)
    return {"radtan": EUROC[0], "radtan_k3": k3, "eucm": TUM_VI[0],
            "eucm_low_alpha": Camera.eucm(190.0, 191.0, 255.0, 257.0, 0.4, 1.1)}


def _ocam(oracle, cam):
    return oracle.camera(cam.model, cam.params, 0, cam.max_iterations)


def _points(n, seed):
    """Camera-frame points in front of, beside and behind the camera; with n >= 8 the special ones."""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(-2, 8, n)], 1)
    if n >= 8:
        p[0] = [0.0, 0.0, 0.0]        # den = 0, Z = 0
        p[1] = [0.3, -0.2, 0.0]       # Z = 0 beside the axis
        p[2] = [0.0, 0.0, -1.0]       # on the axis behind the camera
        p[3] = [0.1, 0.1, -5.0]       # EUCM alpha < 1/2: den < 0
        p[4] = [3.0, 0.0, -1.0]       # EUCM: behind, den > 0 at either alpha
        p[5] = [0.0, 0.0, 2.0]        # the principal point
        p[6] = [-2.5, 1.5, 1e6]       # far on the axis
        p[7] = [1e-300, -1e-300, 1e-300]
    return np.ascontiguousarray(p)


def _same(got, got_ok, want, want_ok):
    assert np.array_equal(got_ok, want_ok)
    assert got[want_ok].tobytes() == want[want_ok].tobytes()     # bit for bit where valid
    assert np.isnan(got[~want_ok]).all()                         # NaN where not


@pytest.mark.parametrize("name", ["radtan", "radtan_k3", "eucm", "eucm_low_alpha"])
@pytest.mark.parametrize("n", [0, 1, 1000])
def test_project_matches_oracle(gpu, oracle, name, n):
    cam = _cams()[name]
    pts = _points(n, 11 + n)
    want, want_ok = oracle.project(_ocam(oracle, cam), pts)
    got, got_ok = cam.project(pts)
    assert got.shape == (n, 2) and got.dtype == np.float64
    _same(got, got_ok, want, want_ok)
    if n == 1000:   # every validity rule is met by the set
        assert want_ok.any() and (~want_ok).any()
        if name == "eucm_low_alpha":
            assert not want_ok[3] and want_ok[4]
        if name == "eucm":
            assert want_ok[2] and not want_ok[0]


@pytest.mark.parametrize("name", ["radtan_k3", "eucm_low_alpha"])
def test_project_device_matches_host_entry(gpu, name):
    import torch
    cam = _cams()[name]
    n = 1000
    pts = _points(n, 7)
    want, want_ok = cam.project(pts)
    d_pts = torch.from_numpy(pts).cuda()
    d_out = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    d_ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    cam.project_device(d_pts.data_ptr(), n, d_out.data_ptr(), d_ok.data_ptr(), s.cuda_stream)
    cam.project_device(d_pts.data_ptr(), 0, d_out.data_ptr(), None, s.cuda_stream)   # n = 0: a no-op
    s.synchronize()
    _same(d_out.cpu().numpy(), d_ok.cpu().numpy().astype(bool), want, want_ok)
