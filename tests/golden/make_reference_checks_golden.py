"""Generates tests/golden/reference_checks.npz and tests/golden/reference_deform_<cfg>.npz: what the reference's own functions compute on the seeded inputs of the tests that
compare this repository with them (signatures, deformation.pth layout, deform_network fwd + bwd, densify / prune, SSIM / L1, SH -> RGB,
the rasterizer pins, plane smoothness), so that those tests run where the reference tree is absent.  Needs the reference tree
(FDGS_REFERENCE_ROOT, default as in oracle/build_ref.py):
    python tests/golden/make_reference_checks_golden.py"""
import importlib
import inspect
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import densify_oracle as DN  # noqa: E402
from oracle import deform_oracle as DF  # noqa: E402
from oracle import loss_oracle as LO  # noqa: E402
from oracle import regulation_oracle as RG  # noqa: E402
from oracle.build_ref import REF  # noqa: E402
import reference_checks as RC  # noqa: E402

fdgs = importlib.import_module("4dgaussians_amd")
syn = fdgs.synthetic
out = {}


def sig(fn):
    return [p.name if p.default is inspect.Parameter.empty else f"{p.name}={p.default!r}" for p in inspect.signature(fn).parameters.values()]


# ---- signatures (tests/test_api_signatures.py)
lu = LO.import_reference_loss_utils()
spec = importlib.util.spec_from_file_location("_ref_image_utils", os.path.join(REF, "utils", "image_utils.py"))
iu = importlib.util.module_from_spec(spec)
spec.loader.exec_module(iu)
GM = DN.import_reference_gaussian_model()
for name, fn in (("l1_loss", lu.l1_loss), ("l2_loss", lu.l2_loss), ("ssim", lu.ssim), ("psnr", iu.psnr), ("mse", iu.mse)):
    out["sig." + name] = np.array(sig(fn), dtype=str)
for name in RC.GM_METHODS:
    out["sig.GaussianModel." + name] = np.array(sig(getattr(GM, name)), dtype=str)

# ---- deformation.pth layout of the reference's deform_network (tests/test_io_formats.py)
RefNet = DF.import_reference_deform_network()
for cfg in RC.DEFORM_CFGS:
    sd = RefNet(syn.deform_args(cfg)).state_dict()
    out[f"layout.{cfg}"] = np.array([RC.layout_entry(k, v) for k, v in sd.items()], dtype=str)

# ---- deform_network forward + backward (tests/test_oracle_deform.py): this repository's seeded network loaded into the reference's,
# at the named configs and at the shapes of RC.DEFORM_SHAPE_CASES
for cfg in RC.DEFORM_CFGS + tuple(RC.DEFORM_SHAPE_CASES):
    args = RC.deform_args(cfg)
    net = RefNet(args)
    net.load_state_dict(RC.seeded_deform_state(cfg), strict=True)
    xyz, sc, rot, op, shs, t = [x.clone().requires_grad_(i < 5) for i, x in enumerate(RC.deform_inputs())]
    res = net(xyz, sc, rot, op, shs, t)
    ws = RC.deform_weights(res)
    params = [(k, p) for k, p in net.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad(sum((a * w).sum() for a, w in zip(res, ws)), [xyz, sc, rot, op, shs] + [p for _, p in params], allow_unused=True)
    dout = {f"deform.{cfg}.out{i}": a.detach().numpy() for i, a in enumerate(res)}
    for name, g in zip(["in.xyz", "in.scales", "in.rot", "in.opacity", "in.shs"] + [k for k, _ in params], grads):
        if g is not None:
            dout[f"deform.{cfg}.grad.{name}"] = g.numpy()
    np.savez_compressed(RC.deform_path(cfg), **dout)
    print(f"{RC.deform_path(cfg)}: {len(dout)} arrays, {os.path.getsize(RC.deform_path(cfg))} bytes")

# ---- densify / prune of the reference's GaussianModel (tests/test_oracle_densify.py)
for i, (n, seed, size) in enumerate(RC.DENSIFY_CASES):
    st = DN.random_state(n, seed, sh_rest=3)
    normals = torch.randn(2 * n, 3, generator=torch.Generator().manual_seed(seed))
    m = DN.reference_model_from_state(st, 0.01)
    with DN.reference_on_cpu(normals):
        m.densify(0.0002, 0.005, 3.0, size, 5, 5)
        RC.save_state(out, f"densify{i}_densified", DN.state_from_reference_model(m))
        m.max_radii2D = torch.rand(m.get_xyz.shape[0], generator=torch.Generator().manual_seed(seed + 1)) * 40
        m.prune(0.0002, 0.05, 3.0, size)
        RC.save_state(out, f"densify{i}_pruned", DN.state_from_reference_model(m))

# ---- SSIM / L1 (tests/test_oracle_loss.py)
for shape in RC.LOSS_SHAPES:
    a, b = RC.loss_inputs(shape)
    a.requires_grad_(True)
    key = "loss." + "x".join(map(str, shape))
    out[key + ".ssim_avg"] = lu.ssim(a, b, size_average=True).detach().numpy()
    out[key + ".ssim_items"] = lu.ssim(a, b, size_average=False).detach().numpy()
    out[key + ".grad_ssim"] = torch.autograd.grad(lu.ssim(a, b), a)[0].numpy()
    out[key + ".l1"] = lu.l1_loss(a, b).detach().numpy()

# ---- SH -> RGB (tests/test_oracle_raster.py) and the rasterizer pins (tests/test_oracle_raster_pins.py)
import utils.general_utils as gu  # noqa: E402  (on sys.path since import_reference_gaussian_model)
from utils.graphics_utils import getProjectionMatrix, getWorld2View2  # noqa: E402
from utils.sh_utils import eval_sh  # noqa: E402
sh, d = RC.sh_inputs()
for deg in range(4):
    out[f"sh.deg{deg}"] = eval_sh(deg, sh.transpose(1, 2), d).numpy()
Z = np.load(os.path.join(HERE, "raster_pins.npz"))
with DN.reference_on_cpu():
    L = gu.build_scaling_rotation(0.7 * torch.tensor(Z["cov.scales"]), torch.tensor(Z["cov.rotations_raw"]))
    out["pins.cov3D.mod0.7"] = gu.strip_symmetric(L @ L.transpose(1, 2)).numpy()
out["pins.cam1.w2v"] = getWorld2View2(Z["cam1.R"], Z["cam1.T"])
cam = syn.make_camera(1352, 1014, theta_deg=-60.0)
out["pins.cam1.proj"] = getProjectionMatrix(0.01, 100.0, cam.FoVx, cam.FoVy).numpy()

# ---- plane smoothness (tests/test_oracle_regulation.py)
smooth = RG.import_reference_plane_smoothness()
for shape in RC.SMOOTH_SHAPES:
    t = RC.smooth_input(shape).requires_grad_(True)
    with RC.one_thread():
        v = smooth(t)
        g = torch.autograd.grad(v, t)[0]
    key = "smooth." + "x".join(map(str, shape))
    out[key + ".value"] = np.array(RC.digest(v))         # (compared bit for bit: the digests say as much as the arrays)
    out[key + ".grad"] = np.array(RC.digest(g))

np.savez_compressed(RC.PATH, **out)
print(f"{RC.PATH}: {len(out)} arrays, {os.path.getsize(RC.PATH)} bytes")
