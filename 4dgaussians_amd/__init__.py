"""MI355X-native 4D-Gaussian render path (hand-written HIP for gfx950 behind the reference's Python API).

The directory name starts with a digit, so import it by string:
    fdgs = importlib.import_module("4dgaussians_amd")          (or `import fdgs`, the root-level alias)
Sub-modules: rasterizer (drop-in for `diff_gaussian_rasterization`), deformation (drop-in `deform_network`),
renderer (`render()` of gaussian_renderer/__init__.py:18; with `pipe.render_alpha = True`, as `GaussianRasterizer(..., render_alpha=True)`, also the accumulated opacity `alpha` [1,H,W], differentiable), regulation (`compute_regulation`, the HexPlane regulariser), losses (`l1_loss`, `ssim`, `psnr`, fused `image_loss`), densify (densification statistics, clone / split / prune with optimizer-state surgery), optim (`FusedAdam`, the multi-tensor optimizer step; `SparseGaussianAdam`, the same stepping only the rows a frame's `visibility_filter` marks), knn (`distCUDA2` of simple-knn), io (PLY point clouds and deformation checkpoints in the reference's formats), parallel (frame-parallel driver), playback (`bake` / `Baked.render`: frames rendered from deformed states resident in device memory; `bake_sparse` / `SparseBaked.render`: the same storing per timestamp only the rows that move, `motion_extent`; `export_ply_sequence`, `to_rgb8`), compose (`compose` / `Composite.render`: several baked models placed in one world by a `Placement` and rasterized once; `sh_rotation`, `map_time`), camera (`PoseDelta`: a camera pose correction to fit, differentiable down to the tensors the rasterizer reads; render() and GaussianRasterizer return the camera's gradient when those tensors require grad; `TimeDelta`: a per-camera time offset to fit, render() and deform() return dL/dt when the time is a tensor that requires grad), synthetic (test scenes).
The HIP library is loaded lazily on first use and there is no CPU fallback.
"""
from . import _lib, camera, compose, deformation, densify, io, knn, losses, optim, parallel, playback, rasterizer, regulation, renderer, sh, synthetic  # noqa: F401
from .deformation import deform_network  # noqa: F401
from .renderer import render, render_views  # noqa: F401
from .regulation import compute_regulation  # noqa: F401
from .optim import FusedAdam, SparseGaussianAdam  # noqa: F401
from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer  # noqa: F401
from .camera import PoseDelta, TimeDelta  # noqa: F401

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "deform_network", "render", "render_views", "compute_regulation", "FusedAdam", "SparseGaussianAdam", "PoseDelta", "TimeDelta", "rasterizer", "regulation", "optim", "losses", "densify",
           "deformation", "renderer", "playback", "compose", "camera", "synthetic", "_lib"]
