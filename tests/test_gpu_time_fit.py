"""Time recovery: "when was this frame taken" against a frozen model.  A fdgs.TimeDelta is fitted with Adam through render()'s time gradient
(fdgs_deform_time_grad) against the image the model gives at t* = 0.43; the yardstick is the same loop in float64 on the CPU through the
oracles oracle/chain.py chains -- oracle.deform_oracle.deform_forward into the dense oracle.raster_torch.rasterize, which (unlike the C
rasterizer oracle of the chain itself) autograd can differentiate down to t.  Run with -m gpu on MI355X.

Scene: 300 Gaussians, 64 x 48, dynerf_default, frozen.  Chosen on the CPU reference before any device run:
  * the start.  From t = 0.40 the float64 reference does NOT approach t*: 0.40 lies two time rows from 0.43 (150 rows: p = 104.3 against
    106.5), the field is piecewise cubic in t with random time planes, and the fit settles in a local minimum of its own cell (0.39857 at
    lr 5e-4 .. 2e-3, 60 .. 100 steps).  The start is therefore 0.425, inside t*'s time cell [0.4228, 0.4362];
  * lr 5e-4, 60 steps: the reference ends at 0.430184 (|t - t*| = 1.8e-4 of a start 5e-3 off), still moving 2.4e-4 over its last 10 steps
    (the sum of |step|) -- the optimiser's distance, not float64's resolution.
The device must end within 3 x that movement of where the reference ends (the margin is taken from the reference run itself).
Measured on MI355X: device 0.430184, |device - reference| = 2.5e-8 against a margin of 7.2e-4."""
import importlib
import math

import pytest
import torch

from oracle import deform_oracle as DO
from oracle import raster_torch

pytestmark = pytest.mark.gpu
T_STAR, T_START, LR, STEPS = 0.43, 0.425, 5e-4, 60
N, W, H, SEED = 300, 64, 48, 21


def _mod():
    return importlib.import_module("4dgaussians_amd")


def _scene():
    syn = _mod().synthetic
    pc = syn.SynthModel(N, "dynerf_default", seed=SEED)
    with torch.no_grad():
        pc._scaling.add_(1.0)
    pc.requires_grad_(False)
    return pc, syn.make_camera(W, H, theta_deg=15.0, time=T_STAR)


def _fit(render, dtype, dev):
    """Adam on a TimeDelta from T_START against render(T_STAR) -> the time after every step.  `render(time tensor) -> color`."""
    with torch.no_grad():
        target = render(torch.tensor(T_STAR, dtype=dtype, device=dev))
    delta = _mod().TimeDelta(dtype=dtype).to(dev)
    opt = torch.optim.Adam(delta.parameters(), lr=LR)
    traj = []
    for _ in range(STEPS):
        opt.zero_grad(set_to_none=True)
        ((render(torch.tensor(T_START, dtype=dtype, device=dev) + delta.offset[0]) - target) ** 2).mean().backward()
        opt.step()
        traj.append(T_START + float(delta.offset.detach()[0]))
    return traj


def _fit_reference():
    pc, cam = _scene()
    dt = torch.float64
    sd = {k: (v.detach().to(dt) if v.dtype.is_floating_point else v) for k, v in pc._deformation.state_dict().items()}
    leaf = {k: getattr(pc, k).detach().to(dt) for k in ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest")}
    shs = torch.cat([leaf["_features_dc"], leaf["_features_rest"]], 1)
    fixed = dict(viewmatrix=cam.world_view_transform.to(dt), projmatrix=cam.full_proj_transform.to(dt), campos=cam.camera_center.to(dt),
                 bg=torch.zeros(3, dtype=dt), image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
                 sh_degree=3)

    def render(t):
        m3, sc, rot, op, sh = DO.deform_forward(sd, pc._deformation.args, leaf["_xyz"], leaf["_scaling"], leaf["_rotation"], leaf["_opacity"], shs,
                                                t.reshape(1, 1).expand(N, 1), activate=True)
        return raster_torch.rasterize(means3D=m3, opacities=op, shs=sh, scales=sc, rotations=rot, **fixed)[0]

    return _fit(render, dt, torch.device("cpu"))


def test_time_recovery_against_the_float64_fit():
    fd = _mod()
    dev = torch.device("cuda:0")
    ref = _fit_reference()
    movement = sum(abs(a - b) for a, b in zip(ref[-10:], ref[-11:-1]))
    assert abs(ref[-1] - T_STAR) < 0.1 * abs(T_START - T_STAR), ("the reference fit itself", ref[-1])
    pc, cam = _scene()
    pc, cam = pc.to(dev), cam.to(dev)
    pipe = type("Pipe", (), dict(convert_SHs_python=False, compute_cov3D_python=False, debug=False))()
    bg = torch.zeros(3, device=dev)

    def render(t):
        cam.time = t
        return fd.render(cam, pc, pipe, bg, stage="fine")["render"]

    got = _fit(render, torch.float32, dev)
    print(f"time recovery after {STEPS} Adam steps (lr {LR}) from {T_START} towards {T_STAR}: float64 reference ends at {ref[-1]:.6f} (moved "
          f"{movement:.2e} over its last 10 steps), device at {got[-1]:.6f}; |device - reference| = {abs(got[-1] - ref[-1]):.2e}, margin {3 * movement:.2e}")
    assert abs(got[-1] - ref[-1]) <= 3 * movement, (got[-1], ref[-1], movement)
    assert abs(got[-1] - T_STAR) < 0.1 * abs(T_START - T_STAR)
