"""Shared by the time-gradient tests (tests/test_time_grad_host.py on the CPU, tests/test_gpu_time_grad.py on the GPU): candidate rows with
planted times, the time-kink filter, fdgs_deform_params over host arrays and the host twin fdgs_deform_time_grad_host."""
import ctypes
import importlib

import numpy as np
import torch

from oracle import deform_oracle as DO
from test_gpu_deform import _net_and_inputs

fdgs = importlib.import_module("4dgaussians_amd")
_lib = fdgs._lib

PLANTED = (0.0, 1.0, 0.5, 1.2)        # times planted on the first rows (in turn): the first / last time row, the clamp beyond it
N_PLANTED = 24
# the safe-row cases of tests/test_gpu_time_grad.py (its comparison with the float64 oracle): (config, rows); scalar: (config, rows, frame time)
ORACLE_CASES = [("dynerf_default", 1531), ("hypernerf_default", 257), ("dnerf_bouncingballs", 1000)]
ORACLE_SCALAR_CASES = [("dynerf_default", 1531, 0.37), ("dnerf_bouncingballs", 1000, 0.613)]


def time_row_distance(t, net):
    """Per row: the least |p - round(p)| over the levels, p = (t + 1) / 2 * (res_t - 1): the distance in texels to a time-row boundary,
    where dL/dt jumps (discontinuity_margin covers ReLU and the spatial cells only)."""
    t = t.reshape(-1).double()
    d = torch.full_like(t, float("inf"))
    for level in net.deformation_net.grid.grids:
        res_t = level[2].shape[2]                   # plane (x, t) is [1, C, res_t, res_x]
        p = (t + 1.0) / 2.0 * (res_t - 1)
        d = torch.minimum(d, (p - torch.round(p)).abs())
    return d


def candidates(cfg, m, seed=3, overrides=None, kplanes=None, fixed_time=None):
    """`m` unfiltered candidate rows of tests/test_gpu_deform.py::_net_and_inputs (time planes = ones + 0.1 randn), with the times of
    PLANTED on the first N_PLANTED rows.  -> (args, net, ins = [xyz, scales, rot, opacity, shs, t])."""
    args, net, ins = _net_and_inputs(cfg, m, seed, None, overrides=overrides, safe=False, fixed_time=fixed_time, kplanes=kplanes)
    if fixed_time is None:
        for i in range(min(N_PLANTED, m)):
            ins[5][i] = PLANTED[i % 4]
    return args, net, ins


def clamped(t):
    return t.reshape(-1) >= 1.0


def time_safe(t, net, margin=1e-4):
    """Rows the tests keep: at least `margin` texels from a time-row boundary at every level -- or clamped (t = 1.0, 1.2), where the
    gradient must be exactly 0."""
    return (time_row_distance(t, net) >= margin) | clamped(t)


def safe_inputs(cfg, n, seed=3, overrides=None, kplanes=None, m=None, relu=True):
    """`n` rows that are safe in time (time_safe) and -- `relu` -- at least 1e-4 from every ReLU kink and spatial cell boundary
    (DO.discontinuity_margin), among them at least one of t = 1.0 and of t = 1.2.  -> (args, net, ins)."""
    m = 4 * n + 256 if m is None else m
    args, net, ins = candidates(cfg, m, seed, overrides, kplanes)
    ok = time_safe(ins[5], net)
    if relu:
        ok &= DO.discontinuity_margin(net.state_dict(), args, ins[0], ins[5]) > 1e-4
    keep = torch.nonzero(ok).squeeze(1)[:n]
    assert keep.numel() == n, f"only {keep.numel()} safe rows among {m} candidates"
    ins = [x[keep].contiguous() for x in ins]
    t = ins[5].reshape(-1)
    assert bool((t == 1.0).any()) and bool((t == 1.2).any()), "the planted clamped rows did not survive the filter"
    return args, net, ins


def safe_inputs_one_time(cfg, n, t, seed=3):
    """`n` rows at ONE frame time `t` (itself at least 1e-4 texels from a time-row boundary) that are at least 1e-4 from every ReLU kink and
    spatial cell boundary.  -> (args, net, ins)."""
    m = 4 * n + 256
    args, net, ins = candidates(cfg, m, seed, fixed_time=t)
    assert float(time_row_distance(ins[5][:1], net)) >= 1e-4
    keep = torch.nonzero(DO.discontinuity_margin(net.state_dict(), args, ins[0], ins[5]) > 1e-4).squeeze(1)[:n]
    assert keep.numel() == n, f"only {keep.numel()} safe rows among {m} candidates"
    return args, net, [x[keep].contiguous() for x in ins]


def host_params(net, xyz, time):
    """fdgs_deform_params over HOST arrays, as fdgs_deform_time_grad_host reads it: `time` a [N,1] / [N] tensor (per-Gaussian) or a float.
    -> (params, the arrays that must outlive it)."""
    grid = net.deformation_net.grid
    p = _lib.DeformParams()
    keep = []
    xyz_np = np.ascontiguousarray(xyz.detach().cpu().numpy(), np.float32)
    keep.append(xyz_np)
    p.N, p.C, p.L, p.W = xyz_np.shape[0], grid.grid_config[0]["output_coordinate_dim"], len(grid.grids), net.deformation_net.W
    for l, level in enumerate(grid.grids):
        for k in range(6):
            a = np.ascontiguousarray(level[k].detach().cpu().permute(0, 2, 3, 1)[0].numpy(), np.float32)      # [H][W][C]
            keep.append(a)
            p.planes[l][k] = a.ctypes.data
        p.res[l][0], p.res[l][1] = level[0].shape[3], level[0].shape[2]
        p.res[l][2], p.res[l][3] = level[5].shape[3], level[5].shape[2]
    for i, v in enumerate(grid.aabb.detach().cpu().reshape(-1).tolist()):
        p.aabb[i] = v
    p.xyz = xyz_np.ctypes.data
    if isinstance(time, torch.Tensor):
        t_np = np.ascontiguousarray(time.detach().cpu().reshape(-1).numpy(), np.float32)
        keep.append(t_np)
        p.time = t_np.ctypes.data
    else:
        p.time, p.time_scalar = None, float(time)
    return p, keep


def host_twin(p, dfeat, live):
    """fdgs_deform_time_grad_host -> (rows float64 [N], sum, sum |addend| per row [N], sum |addend|)."""
    n = p.N
    dfeat = np.ascontiguousarray(dfeat, np.float32)
    live = np.ascontiguousarray(live, np.uint8)
    rows, arows = np.zeros(n, np.float64), np.zeros(n, np.float64)
    tot, atot = ctypes.c_double(), ctypes.c_double()
    _lib.check(_lib.lib().fdgs_deform_time_grad_host(p, dfeat.ctypes.data, live.ctypes.data, rows.ctypes.data, ctypes.addressof(tot),
                                                     arows.ctypes.data, ctypes.addressof(atot)))
    return rows, tot.value, arows, atot.value


def oracle_dt(net, xyz, t, dfeat, dtype=torch.float64):
    """d sum(features * dfeat) / dt per row through oracle.deform_oracle.hexplane_features' autograd, evaluated in `dtype`."""
    sd = {k: (v.detach().to(dtype) if v.dtype.is_floating_point else v) for k, v in net.state_dict().items()}
    tt = t.detach().reshape(-1, 1).to(dtype).requires_grad_(True)
    feat = DO.hexplane_features(sd, xyz.detach().to(dtype), tt, DO.count_levels(sd))
    g, = torch.autograd.grad((feat * torch.as_tensor(dfeat).to(dtype)).sum(), tt)
    return g.reshape(-1).double().numpy()


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
