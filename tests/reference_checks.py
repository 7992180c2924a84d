"""Seeded inputs shared by tests/golden/make_reference_checks_golden.py (which evaluates the reference's own functions on them) and the
tests that compare this repository with those results (tests/golden/reference_checks.npz): one definition, so both sides see the same
cases."""
import contextlib
import hashlib
import importlib
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATH = os.path.join(GOLD, "reference_checks.npz")

GM_METHODS = ("add_densification_stats", "prune_points", "prune", "reset_opacity", "densify", "save_ply", "load_ply", "save_deformation",
              "load_model", "compute_regulation")
DEFORM_CFGS = ("dnerf_bouncingballs", "hypernerf_default", "dynerf_default")
# deform_network shapes that no named config has: name -> (config it starts from, overrides of synthetic.deform_args, kplanes_config entries).
# "refdefaults": the reference's own argument defaults (arguments/__init__.py: net_width 64, defor_depth 1, output_coordinate_dim 32,
# multires [1, 2, 4, 8], position / scale / rotation heads); the other: net_width 128 at C * L = 96 with a head set no config has.  The base
# resolution is small so that the recorded plane gradients stay below the largest file of tests/golden.
DEFORM_SHAPE_CASES = {
    "refdefaults": ("dnerf_bouncingballs", dict(net_width=64, defor_depth=1, multires=[1, 2, 4, 8]),
                    dict(output_coordinate_dim=32, resolution=[16, 16, 16, 10])),
    "w128_f96_heads_x_o_shs": ("dynerf_default", dict(net_width=128, defor_depth=0, multires=[1, 2, 4], no_ds=True, no_dr=True),
                               dict(output_coordinate_dim=32, resolution=[16, 16, 16, 10])),
}
DENSIFY_CASES = ((300, 3, 20), (64, 4, None), (1, 5, 20))
LOSS_SHAPES = ((1, 3, 11, 11), (2, 3, 40, 64), (1, 1, 5, 70))
SMOOTH_SHAPES = ((1, 16, 75, 64), (1, 32, 3, 5), (2, 4, 10, 7))
DEFORM_N = 33           # (the grids' gradients of the recorded deform_network cases grow with it)

_Z = {}


def deform_path(cfg):
    """The deform_network case of `cfg` lives in a file of its own (like tests/golden/deform_<cfg>.npz)."""
    return os.path.join(GOLD, f"reference_deform_{cfg}.npz")


def load(path=PATH):
    if path not in _Z:
        _Z[path] = np.load(path)
    return _Z[path]


def digest(a):
    """sha256 of shape, dtype and bytes: equal digests <=> bit-identical arrays (what torch.equal asserts, -0.0 vs 0.0 told apart)."""
    a = np.ascontiguousarray(a.detach().numpy() if isinstance(a, torch.Tensor) else a)
    return hashlib.sha256(f"{a.shape}|{a.dtype}|".encode() + a.tobytes()).hexdigest()


def layout_entry(key, value):
    return f"{key}|{tuple(value.shape)}|{value.dtype}"


def deform_inputs():
    """xyz, scales, rotations, opacity, shs, t of DEFORM_N Gaussians."""
    g = importlib.import_module("4dgaussians_amd.synthetic").make_gaussians(DEFORM_N, seed=1)
    shs = torch.cat([g["features_dc"], g["features_rest"]], 1)
    t = torch.rand(DEFORM_N, 1, generator=torch.Generator().manual_seed(7))
    return g["xyz"], g["scaling"], g["rotation"], g["opacity"], shs, t


def deform_args(cfg):
    """The deform_network arguments of a named config or of one of DEFORM_SHAPE_CASES."""
    syn = importlib.import_module("4dgaussians_amd.synthetic")
    if cfg not in DEFORM_SHAPE_CASES:
        return syn.deform_args(cfg)
    base, overrides, kplanes = DEFORM_SHAPE_CASES[cfg]
    args = syn.deform_args(base, **overrides)
    args.kplanes_config.update(kplanes)
    return args


def seeded_deform_state(cfg):
    """State dict of this repository's deform_network for `cfg` (seeded, HexPlane grids perturbed, aabb of deform_inputs())."""
    fdgs = importlib.import_module("4dgaussians_amd")
    torch.manual_seed(6666)
    net = fdgs.deform_network(deform_args(cfg))
    gen = torch.Generator().manual_seed(6667)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if "grids" in name:
                p.add_(0.1 * torch.randn(p.shape, generator=gen))
    xyz = deform_inputs()[0]
    net.deformation_net.set_aabb(xyz.max(0).values.tolist(), xyz.min(0).values.tolist())
    return net.state_dict()


def deform_weights(outs):
    gen = torch.Generator().manual_seed(8)
    return [torch.randn(a.shape, generator=gen) for a in outs]


def save_state(out, prefix, st):
    for k, v in st.items():
        if isinstance(v, dict):
            for n, t in v.items():
                out[f"{prefix}.{k}.{n}"] = t.detach().numpy()
        else:
            out[f"{prefix}.{k}"] = v.detach().numpy()


def loss_inputs(shape):
    gen = torch.Generator().manual_seed(sum(shape))
    return torch.rand(*shape, generator=gen), torch.rand(*shape, generator=gen)


def sh_inputs():
    rng = np.random.default_rng(0)
    sh = torch.tensor(rng.standard_normal((20, 16, 3)))
    d = torch.nn.functional.normalize(torch.tensor(rng.standard_normal((20, 3))), dim=1)
    return sh, d


def smooth_input(shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(3))


@contextlib.contextmanager
def one_thread():
    """Single-threaded CPU reductions: results that are compared bit for bit do not depend on the host's core count."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)
