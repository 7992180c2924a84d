"""Camera pose as something to fit: a small correction of a camera's pose, differentiable down to the three tensors the rasterizer reads.

render(), GaussianRasterizer and the C ABI return dL/d(viewmatrix, projmatrix, campos) when any of the three requires grad
(rasterizer.camera_wants_grad; csrc/preprocess.hip fdgs_camera_grad).  `PoseDelta` is the parametrisation in front of them: six numbers
per camera, zero = the camera as it is.  The chain from the three tensors' gradients to the six numbers is torch's.

    delta = PoseDelta().to(device)
    opt = torch.optim.Adam(delta.parameters(), lr=1e-3)
    out = render(delta.pose(cam), gaussians, pipe, background)         # or GaussianRasterizer(delta.settings(...)) for the raw route
    loss(out["render"], target).backward()                             # model and pose gradients from the same backward

The frame time is the other thing a camera can be wrong about.  render() and deform() return dL/dt when the time is a tensor that requires
grad (csrc/deform_time_grad.h, fdgs_deform_time_grad); `TimeDelta` is the parametrisation in front of it: one offset per camera, zero = the
camera's own time.  The two compose: `TimeDelta.camera(PoseDelta.pose(cam))` is a camera whose pose and time are both being fitted.
"""
import torch
import torch.nn as nn


class PosedCamera:
    """What render() reads of a camera, with the three pose tensors computed by PoseDelta.pose (they carry the graph)."""
    __slots__ = ("image_height", "image_width", "FoVx", "FoVy", "time", "world_view_transform", "full_proj_transform", "camera_center",
                 "projection_matrix")

    def __init__(self, **fields):
        for k in self.__slots__:
            setattr(self, k, fields[k])


def _skew(w):
    z = w.new_zeros(())
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


class PoseDelta(nn.Module):
    """A perturbation of a camera in the camera's own frame: p_view' = exp(omega) p_view + tau, `omega` [3] axis-angle (radians), `tau` [3]
    in scene units.  Zero parameters are the identity.  In the project's row-vector convention (p_view = (p, 1) @ V, matrices row-major)
    that is V' = V @ D with D = [[exp(omega)^T, 0], [tau, 1]]."""

    def __init__(self, dtype=torch.float32):
        super().__init__()
        self.omega = nn.Parameter(torch.zeros(3, dtype=dtype))
        self.tau = nn.Parameter(torch.zeros(3, dtype=dtype))

    def matrix(self):
        """D [4,4] (row-vector convention).  exp through torch.matrix_exp: smooth at omega = 0, where the closed form divides 0 by 0."""
        E = torch.matrix_exp(_skew(self.omega))
        top = torch.cat([E.t(), E.new_zeros(3, 1)], 1)
        bottom = torch.cat([self.tau, self.tau.new_ones(1)]).unsqueeze(0)
        return torch.cat([top, bottom], 0)

    def transforms(self, world_view_transform, full_proj_transform, projection_matrix=None):
        """(world_view_transform', full_proj_transform', camera_center') of the perturbed camera, differentiable in omega and tau:
        V' = V @ D, full_proj' = V' @ P with P the camera's projection matrix (None: solve(V, full_proj)), camera_center' = inverse(V')[3, :3]."""
        like = dict(device=self.omega.device, dtype=self.omega.dtype)
        V = world_view_transform.detach().to(**like).reshape(4, 4)
        if projection_matrix is not None:
            P = projection_matrix.detach().to(**like).reshape(4, 4)
        else:
            P = torch.linalg.solve(V, full_proj_transform.detach().to(**like).reshape(4, 4))
        Vp = V @ self.matrix()
        return Vp, Vp @ P, torch.linalg.inv(Vp)[3, :3]

    def pose(self, camera):
        """`camera` (anything with the fields render() reads) moved by this correction -> PosedCamera."""
        V, F, c = self.transforms(camera.world_view_transform, camera.full_proj_transform, getattr(camera, "projection_matrix", None))
        return PosedCamera(image_height=camera.image_height, image_width=camera.image_width, FoVx=camera.FoVx, FoVy=camera.FoVy,
                           time=camera.time, world_view_transform=V, full_proj_transform=F, camera_center=c,
                           projection_matrix=getattr(camera, "projection_matrix", None))

    def settings(self, raster_settings):
        """The raw route: a GaussianRasterizationSettings whose viewmatrix, projmatrix and campos are this correction's."""
        V, F, c = self.transforms(raster_settings.viewmatrix, raster_settings.projmatrix)
        return raster_settings._replace(viewmatrix=V, projmatrix=F, campos=c)


class TimeDelta(nn.Module):
    """A time offset per camera: cameras that are not frame-synchronised, jittered timestamps, or "when was this photo taken" against a
    frozen model.  `offset` [n_cameras], zero = the camera's own time."""

    def __init__(self, n_cameras=1, dtype=torch.float32):
        super().__init__()
        self.offset = nn.Parameter(torch.zeros(n_cameras, dtype=dtype))

    def camera(self, camera, index=0):
        """`camera` (anything with the fields render() reads, a PosedCamera of PoseDelta.pose included) at time + offset[index] ->
        PosedCamera whose `time` is a 0-dim tensor that carries the graph; everything else is the camera's own."""
        t = camera.time
        if not isinstance(t, torch.Tensor):
            t = torch.tensor(float(t), dtype=self.offset.dtype, device=self.offset.device)
        time = t.to(device=self.offset.device, dtype=self.offset.dtype).reshape(()) + self.offset[index]
        return PosedCamera(image_height=camera.image_height, image_width=camera.image_width, FoVx=camera.FoVx, FoVy=camera.FoVy, time=time,
                           world_view_transform=camera.world_view_transform, full_proj_transform=camera.full_proj_transform,
                           camera_center=camera.camera_center, projection_matrix=getattr(camera, "projection_matrix", None))
