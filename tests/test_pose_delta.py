"""fdgs.camera.PoseDelta against torch alone (CPU): zero is the identity, the camera centre is the inverse's, and autograd's gradients of
the three tensors with respect to the six numbers pass gradcheck in float64."""
import importlib
import math

import torch

fdgs = importlib.import_module("4dgaussians_amd")
syn = fdgs.synthetic
PoseDelta = fdgs.camera.PoseDelta


def _cam():
    return syn.make_camera(64, 48, theta_deg=25.0, time=0.3)


def test_zero_parameters_reproduce_the_camera():
    cam = _cam()
    posed = PoseDelta().pose(cam)
    assert torch.allclose(posed.world_view_transform, cam.world_view_transform, rtol=0, atol=1e-6)
    assert torch.allclose(posed.full_proj_transform, cam.full_proj_transform, rtol=0, atol=1e-5)
    assert torch.allclose(posed.camera_center, cam.camera_center, rtol=0, atol=1e-5)
    for k in ("image_height", "image_width", "FoVx", "FoVy", "time"):
        assert getattr(posed, k) == getattr(cam, k)
    # without a projection_matrix: P = solve(V, full_proj)
    V, F, c = PoseDelta().transforms(cam.world_view_transform, cam.full_proj_transform)
    assert torch.allclose(F, cam.full_proj_transform, rtol=0, atol=1e-5) and torch.allclose(c, cam.camera_center, rtol=0, atol=1e-5)


def test_the_perturbation_is_in_the_camera_frame_and_the_centre_is_the_inverses():
    cam = _cam()
    d = PoseDelta(dtype=torch.float64)
    with torch.no_grad():
        d.omega.copy_(torch.tensor([0.03, -0.02, 0.05]))
        d.tau.copy_(torch.tensor([0.1, -0.2, 0.05]))
    V, F, c = d.transforms(cam.world_view_transform, cam.full_proj_transform, getattr(cam, "projection_matrix", None))
    assert torch.allclose(c, torch.linalg.inv(V)[3, :3], rtol=0, atol=1e-12)
    # p_view' = exp(omega) p_view + tau for a world point (row-vector convention)
    p = torch.tensor([0.3, -0.4, 0.2, 1.0], dtype=torch.float64)
    pv, pv2 = (p @ cam.world_view_transform.double())[:3], (p @ V)[:3]
    w = d.omega.detach()
    th = w.norm()
    k = w / th
    rod = pv * math.cos(th) + torch.linalg.cross(k, pv) * math.sin(th) + k * (k @ pv) * (1 - math.cos(th))       # Rodrigues
    assert torch.allclose(pv2, rod + d.tau.detach(), rtol=0, atol=1e-12)
    # the camera centre maps to the view-space origin
    assert torch.allclose((torch.cat([c, c.new_ones(1)]) @ V)[:3], torch.zeros(3, dtype=torch.float64), atol=1e-12)
    # full_proj' = V' @ P
    P = torch.linalg.solve(cam.world_view_transform.double(), cam.full_proj_transform.double())
    assert torch.allclose(F, V @ P, rtol=0, atol=1e-9)


def test_gradcheck():
    cam = _cam()
    d = PoseDelta(dtype=torch.float64)

    def f(omega, tau):
        d.omega.data, d.tau.data = omega.data, tau.data
        d._parameters["omega"], d._parameters["tau"] = omega, tau
        return d.transforms(cam.world_view_transform, cam.full_proj_transform)

    for om in ([0.0, 0.0, 0.0], [0.03, -0.02, 0.05]):
        omega = torch.tensor(om, dtype=torch.float64, requires_grad=True)
        tau = torch.tensor([0.1, -0.2, 0.05], dtype=torch.float64, requires_grad=True)
        assert torch.autograd.gradcheck(f, (omega, tau), eps=1e-6, atol=1e-7)
