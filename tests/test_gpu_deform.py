"""GPU parity tests of the fused HIP deformation (HexPlane + MLP, fwd + bwd) and of render() end to end, against the
CPU oracle (which is itself pinned to the reference's modules, tests/test_oracle_deform.py)."""
import importlib
import math

import numpy as np
import pytest

from conftest import set_knob
import torch

from oracle import deform_oracle as DO
from oracle.raster_oracle import RasterOracle
from scenes import rel_l2

pytestmark = pytest.mark.gpu
synthetic = importlib.import_module("4dgaussians_amd.synthetic")


def _fdgs():
    return importlib.import_module("4dgaussians_amd")


def _net_and_inputs(cfg, n, seed, dev, overrides=None, safe=True, fixed_time=None, candidates=None, kplanes=None):
    """`overrides`: fields of synthetic.deform_args; `kplanes`: entries of its kplanes_config (output_coordinate_dim, resolution);
    `candidates`: rows drawn before the safe ones are picked (default 2n + 64; the share of safe rows falls with net_width and levels)."""
    fd = _fdgs()
    torch.manual_seed(seed)
    args = synthetic.deform_args(cfg, **(overrides or {}))
    args.kplanes_config.update(kplanes or {})
    net = fd.deform_network(args)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if "grids" in name:
                p.add_(0.1 * torch.randn(p.shape, generator=gen))
    m = (2 * n + 64 if candidates is None else candidates) if safe else n
    g = synthetic.make_gaussians(m, seed=seed)
    xyz = g["xyz"] * 1.05  # a few points outside the aabb: border clamp + zero coordinate gradient
    net.deformation_net.set_aabb([1.3, 1.25, 1.2], [-1.3, -1.2, -1.25])
    shs = torch.cat([g["features_dc"], g["features_rest"]], 1)
    t = torch.rand(m, 1, generator=gen)
    t[:4] = torch.tensor([[0.0], [1.0], [0.5], [1.2]])
    if fixed_time is not None:
        t[:] = float(fixed_time)
    ins = [xyz, g["scaling"], g["rotation"], g["opacity"], shs, t]
    if safe:
        # keep Gaussians that sit at least 1e-4 away from every ReLU kink / texel boundary: there float32 rounding
        # (GPU fmaf chain vs CPU sgemm) cannot flip a derivative, so gradients can be compared tightly
        margin = DO.discontinuity_margin(net.state_dict(), args, xyz, t)
        keep = torch.nonzero(margin > 1e-4).squeeze(1)[:n]
        assert keep.numel() == n, f"only {keep.numel()} safe Gaussians"
        ins = [x[keep].contiguous() for x in ins]
    return args, net, ins


CFGS = [("dnerf_bouncingballs", 1000), ("hypernerf_default", 257), ("dynerf_default", 1531),
        ("dynerf_default", 31)]


@pytest.mark.parametrize("cfg,n", CFGS)
@pytest.mark.parametrize("activate", [False, True])
def test_deform_forward_backward_parity(cfg, n, activate):
    _parity(cfg, n, activate)


@pytest.mark.parametrize("cfg,n,t", [("dnerf_bouncingballs", 1000, None), ("hypernerf_default", 257, None), ("dynerf_default", 1531, None),
                                     ("dynerf_default", 31, None), ("dynerf_default", 40100, 0.37), ("hypernerf_default", 5000, 1.0)])
@pytest.mark.parametrize("form", ["8", "16", "32"])
def test_deform_parity_other_forms_of_the_forward_kernel(cfg, n, t, form):
    """The forms of the forward kernel that are NOT the default.  (Default since round 6: d1_form = 0 picks by shape -- the WEIGHT-STATIONARY form 8 at net_width 128 with up to two HexPlane
    levels, form 16 otherwise; every form is forced here on every config.  d1_form = 8: the weight-stationary form of csrc/deform_fwd_ws.h -- the waves of a workgroup hold the heads' first-layer matrices in
    registers, 16-Gaussian tiles visit them through LDS, the gather is a kernel of its own.)
    d1_form = 16: one wave = 16 Gaussians on v_mfma_f32_16x16x4_f32, two waves per SIMD, W0 / W1 read as packed operand streams (the default
    of rounds 4 - 5); d1_form = 32: one wave = 32 Gaussians on v_mfma_f32_32x32x2_f32, one wave per SIMD (the default until round 4, and what
    the library runs when the caller hands over no scratch or C*L is not a multiple of 16) -- same oracle, same tolerances, forward AND the
    backward that consumes its saved activations and ReLU bit masks; sizes with a partial last tile, a single tile, and the leftover-tile
    split of the persistent loops."""
    set_knob("d1_form", form)
    _parity(cfg, n, True, scalar_time=t)


@pytest.mark.parametrize("form", ["16", "32"])
def test_deform_parity_leftover_tiles_split_by_head(form):
    """The persistent loop of the forward kernel deals the tiles left over after its last full round out BY HEAD over the waves.  At test
    sizes that branch is only taken with a small grid: 5 000 Gaussians on 13 workgroups leave 8 of 320 tiles (form 16) / 4 of 160 tiles
    (form 32) for the split round."""
    set_knob("d1_form", form)
    set_knob("d1_wgs", "13")
    _parity("dynerf_default", 5000, True, scalar_time=0.61)


@pytest.mark.parametrize("cfg,n,t", [("dynerf_default", 2100, 0.37), ("hypernerf_default", 700, 1.0), ("dnerf_bouncingballs", 900, 0.0)])
def test_deform_parity_one_frame_time(cfg, n, t):
    """render() hands ONE frame time to all Gaussians: the plane-gradient kernel then privatises the three time planes in
    LDS (csrc/deform.hip D4).  Same tight comparison as above, including t on the first/last time row (border clamp)."""
    _parity(cfg, n, True, scalar_time=t)


@pytest.mark.parametrize("cfg,n", [("dynerf_default", 1200), ("hypernerf_default", 300)])
def test_deform_parity_recompute_path(cfg, n, monkeypatch):
    """The backward without saved activations (fdgs_deform_out::saved = NULL): gather, trunk and the heads' hidden layers
    are recomputed inside the backward kernel."""
    monkeypatch.setattr(_fdgs().deformation, "SAVE_ACTIVATIONS", False)
    _parity(cfg, n, True)


def _parity_cpu_side(cfg, n, activate, scalar_time, overrides, kplanes, candidates):
    """The CPU half of _parity: network, safe inputs, the oracle's outputs and its gradients of sum(out * w)."""
    dev = torch.device("cuda:0")
    args, net, ins = _net_and_inputs(cfg, n, 3, dev, overrides=overrides, fixed_time=scalar_time, candidates=candidates, kplanes=kplanes)
    # oracle on CPU with the same state dict
    sd = {k: v.detach().clone().contiguous().requires_grad_(v.dtype.is_floating_point and "poc" not in k and "aabb" not in k)
          for k, v in net.state_dict().items()}
    cpu_in = [x.clone().requires_grad_(i < 5) for i, x in enumerate(ins)]
    ref = DO.deform_forward(sd, args, *cpu_in, activate=activate)
    gen = torch.Generator().manual_seed(11)
    ws = [torch.randn(b.shape, generator=gen) for b in ref]
    loss_ref = sum((a * w).sum() for a, w in zip(ref, ws))
    params_cpu = [sd[k] for k in sd if sd[k].requires_grad]
    pnames = [k for k in sd if sd[k].requires_grad]
    g_ref = torch.autograd.grad(loss_ref, cpu_in[:5] + params_cpu, allow_unused=True)
    return dict(args=args, net=net.to(dev), ins=ins, ref=[b.detach() for b in ref], ws=ws, pnames=pnames, g_ref=g_ref)


def _parity(cfg, n, activate, scalar_time=None, overrides=None, kplanes=None, candidates=None, ordered=None, shared=None, details=None):
    """HIP forward and backward against the CPU oracle: outputs to rel-L2 < 2e-5, every gradient of sum(out * w) on safe rows to < 1e-4.
    `overrides`, `kplanes`, `candidates`: see _net_and_inputs; `ordered`: handed to deform().  `shared`: a dict that keeps the CPU half (network,
    inputs, oracle results: read-only) for further calls with the same arguments before it; `details`: a dict that receives the
    forward's per-output rel-L2 ("fwd"), the network ("net"), the inputs ("ins") and the HIP outputs ("out") and gradients ("grads",
    by name, on the CPU).  Returns the per-tensor rel-L2 of the gradients."""
    dev = torch.device("cuda:0")
    fd = _fdgs()
    cpu = shared.get("cpu") if shared is not None else None
    if cpu is None:
        cpu = _parity_cpu_side(cfg, n, activate, scalar_time, overrides, kplanes, candidates)
        if shared is not None:
            shared["cpu"] = cpu
    net, ins, ref, ws, pnames, g_ref = cpu["net"], cpu["ins"], cpu["ref"], cpu["ws"], cpu["pnames"], cpu["g_ref"]
    gpu_in = [x.to(dev).requires_grad_(i < 5) for i, x in enumerate(ins)]
    out = fd.deformation.deform(net, *gpu_in[:4], shs=gpu_in[4], time=gpu_in[5] if scalar_time is None else float(scalar_time),
                                activate=activate, ordered=ordered)
    torch.cuda.synchronize()
    names = ("xyz", "scales", "rot", "opacity", "shs")
    fwd = {k: rel_l2(a.detach().cpu().numpy(), b.numpy().reshape(a.shape)) for k, a, b in zip(names, out, ref)}
    if details is not None:
        details.update(fwd=fwd, net=net, ins=ins, out=[a.detach() for a in out])
    for k, e in fwd.items():
        assert e < 2e-5, (k, e)
    loss = sum((a * w.to(dev).reshape(a.shape)).sum() for a, w in zip(out, ws))
    params_gpu = [dict(net.named_parameters())[k] for k in pnames]
    g_gpu = torch.autograd.grad(loss, gpu_in[:5] + params_gpu, allow_unused=True)
    if details is not None:
        details["grads"] = {k: (None if a is None else a.cpu()) for k, a in zip(list(names) + pnames, g_gpu)}
    report = {}
    for k, a, b in zip(list(names) + pnames, g_gpu, g_ref):
        if b is None:
            assert a is None or float(a.abs().max()) == 0.0, k
            continue
        assert a is not None, k
        report[k] = rel_l2(a.cpu().numpy(), b.numpy().reshape(a.shape))
    worst = sorted(report.items(), key=lambda kv: -kv[1])[:4]
    print(f"[{cfg} n={n} act={activate}] worst grad rel-L2: " + ", ".join(f"{k}={v:.2e}" for k, v in worst))
    for k, a, b in zip(list(names) + pnames, g_gpu, g_ref):
        if b is not None and report.get(k, 0) >= 1e-4:  # diagnostics: is the error confined to a few rows?
            A, B = a.cpu().numpy().reshape(a.shape[0], -1), b.numpy().reshape(a.shape[0], -1)
            rowerr = np.linalg.norm(A - B, axis=1) / (np.linalg.norm(B) / math.sqrt(A.shape[0]) + 1e-30)
            bad = np.argsort(-rowerr)[:5]
            print(f"   {k}: rows with largest error {bad.tolist()} -> {np.round(rowerr[bad], 4).tolist()}")
    for k, v in report.items():
        assert v < 1e-4, (k, v)
    return report


def _grads_pair(cfg, n, seed, upstream_mask=None):
    """HIP and oracle gradients of sum(out * w) on UNFILTERED random inputs; `upstream_mask` [n] zeroes w for some rows."""
    dev = torch.device("cuda:0")
    fd = _fdgs()
    args, net, ins = _net_and_inputs(cfg, n, seed, dev, safe=False)
    sd = {k: v.detach().clone().contiguous().requires_grad_(v.dtype.is_floating_point and "poc" not in k and "aabb" not in k)
          for k, v in net.state_dict().items()}
    margin = DO.discontinuity_margin(net.state_dict(), args, ins[0], ins[5], parts=True)[0]     # the ReLU part alone
    cpu_in = [x.clone().requires_grad_(i < 5) for i, x in enumerate(ins)]
    ref = DO.deform_forward(sd, args, *cpu_in, activate=True)
    net = net.to(dev)
    gpu_in = [x.to(dev).requires_grad_(i < 5) for i, x in enumerate(ins)]
    out = fd.deformation.deform(net, *gpu_in[:4], shs=gpu_in[4], time=gpu_in[5], activate=True)
    for a, b in zip(out, ref):
        assert rel_l2(a.detach().cpu().numpy(), b.detach().numpy().reshape(a.shape)) < 2e-5
    ws = [torch.randn(b.shape, generator=torch.Generator().manual_seed(1)) for b in ref]
    if upstream_mask is not None:
        ws = [w * upstream_mask.reshape([-1] + [1] * (w.dim() - 1)).to(w.dtype) for w in ws]
    pn = [k for k in sd if sd[k].requires_grad]
    g_ref = torch.autograd.grad(sum((a * w).sum() for a, w in zip(ref, ws)), cpu_in[:5] + [sd[k] for k in pn], allow_unused=True)
    g_gpu = torch.autograd.grad(sum((a * w.to(dev).reshape(a.shape)).sum() for a, w in zip(out, ws)),
                                gpu_in[:5] + [dict(net.named_parameters())[k] for k in pn], allow_unused=True)
    names = ["xyz", "scales", "rot", "opacity", "shs"] + pn
    return names, g_gpu, g_ref, margin


@pytest.mark.parametrize("cfg,n", [("dynerf_default", 3000), ("dynerf_default", 60000), ("hypernerf_default", 20000)])
def test_deform_unfiltered_inputs_flips_counted(cfg, n):
    """Unfiltered random inputs, north_star tolerance (1e-3), no pre-filtering of the comparison set.

    The deformation's derivative is discontinuous where a ReLU input crosses 0 or a HexPlane coordinate crosses a texel
    boundary.  A Gaussian whose pre-activation sits within float rounding of 0 can fall on different sides in the GPU's MFMA chain
    and the CPU's sgemm: its forward value is unaffected (the function is continuous) but its gradient contribution flips.
    The texel cell is NOT such a case: the kernels' index arithmetic equals the oracle's float32 operations one for one
    (csrc/hexplane_ops.h, tests/test_gpu_hexplane_cells.py), so the distance to a texel boundary excuses nothing here.
    This test QUANTIFIES the ReLU flips instead of loosening the tolerance:
      1. at-risk rows = Gaussians whose oracle margin to the nearest ReLU kink is < 4e-6; their number must stay below a stated
         bound (they are a property of the inputs, not of the kernel);
      2. with the full upstream gradient, the per-Gaussian input gradients of HIP and oracle may only disagree (> 1e-3 of the
         row scale) on at-risk rows -- every flip is explained -- and the count of such rows is bounded;
      3. with the upstream gradient of the at-risk rows set to zero (their contribution vanishes on both sides whichever way
         they flip) EVERY gradient, including all weight and plane gradients, agrees to 1e-3 rel-L2."""
    names, g_gpu, g_ref, margin = _grads_pair(cfg, n, 9)
    risky = (margin < 4e-6).numpy()
    n_relu = n * (1 + 5) * 128
    bound = max(8, int(4e-5 * n_relu))           # density of pre-activations near 0 is O(1): expect ~ 1e-5 * n_relu
    assert risky.sum() <= bound, f"{risky.sum()} at-risk rows of {n}"
    flipped = np.zeros(n, bool)
    for k, a, b in zip(names[:5], g_gpu[:5], g_ref[:5]):
        A, B = a.cpu().numpy().reshape(n, -1), b.numpy().reshape(n, -1)
        scale = np.linalg.norm(B) / math.sqrt(n) + 1e-30
        flipped |= np.linalg.norm(A - B, axis=1) / scale > 1e-3
    print(f"[{cfg} n={n}] at-risk rows {int(risky.sum())}, rows whose input gradient differs {int(flipped.sum())} (bound {bound})")
    assert not np.any(flipped & ~risky), f"{int((flipped & ~risky).sum())} rows differ without being near a kink"
    assert flipped.sum() <= bound
    names, g_gpu, g_ref, _ = _grads_pair(cfg, n, 9, upstream_mask=torch.tensor(~risky))
    worst = {}
    for k, a, b in zip(names, g_gpu, g_ref):
        if b is not None:
            worst[k] = rel_l2(a.cpu().numpy(), b.numpy().reshape(a.shape))
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:3]
    print("   masked-upstream worst rel-L2: " + ", ".join(f"{k}={v:.2e}" for k, v in top))
    for k, v in worst.items():
        assert v < 1e-3, (k, v)


GOLD = __import__("os").path.join(__import__("os").path.dirname(__file__), "golden")


@pytest.mark.parametrize("cfg", ["dnerf_bouncingballs", "hypernerf_default", "dynerf_default"])
def test_deform_matches_reference_golden_vectors(cfg):
    """The HIP deformation against the fixtures generated by the REFERENCE's own modules (tests/golden/make_deform_golden.py):
    the reference state_dict loads strictly into this package's deform_network, forward outputs and the gradients of
    sum(out * w) w.r.t. every input and every parameter are compared with the stored reference results directly."""
    dev = torch.device("cuda:0")
    fd = _fdgs()
    z = np.load(__import__("os").path.join(GOLD, f"deform_{cfg}.npz"))
    args = synthetic.deform_args(cfg)
    args.kplanes_config["resolution"] = [8, 8, 8, 6]          # the fixtures' (small) plane resolution
    net = fd.deform_network(args)
    missing = net.load_state_dict({k[3:]: torch.tensor(z[k]) for k in z.files if k.startswith("sd.")}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    net = net.to(dev)
    keys = ("xyz", "scales", "rot", "opacity", "shs")
    ins = [torch.tensor(z["in." + k], device=dev).requires_grad_(True) for k in keys]
    t = torch.tensor(z["in.t"], device=dev)
    out = net(*ins, t)
    for k, o in zip(keys, out):
        assert rel_l2(o.detach().cpu().numpy(), z["out." + k]) < 2e-5, k
    loss = sum((o * torch.tensor(z["w." + k], device=dev)).sum() for k, o in zip(keys, out))
    gk = [k for k in z.files if k.startswith("grad.")]
    named = dict(net.named_parameters())
    wanted = [ins[keys.index(k[8:])] if k.startswith("grad.in.") else named[k[8:]] for k in gk]
    grads = torch.autograd.grad(loss, wanted, allow_unused=True)
    worst = {}
    for k, g in zip(gk, grads):
        assert g is not None, k
        worst[k] = rel_l2(g.cpu().numpy(), z[k])
    print(f"[golden {cfg}] worst: " + ", ".join(f"{k}={v:.1e}" for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:3]))
    for k, v in worst.items():
        assert v < 1e-3, (k, v)       # 96 unfiltered Gaussians: north_star tolerance


def test_backward_with_unused_outputs_and_no_grad_forward():
    """(a) Only some outputs reach the loss: autograd hands None for the others (set_materialize_grads(False)) and the
    kernels skip them -- gradients must equal the oracle's for the same partial loss.  (b) Under torch.no_grad() the forward
    neither allocates the saved-activation buffer nor takes the saving path."""
    dev = torch.device("cuda:0")
    fd = _fdgs()
    args, net, ins = _net_and_inputs("dynerf_default", 700, 4, dev)
    sd = {k: v.detach().clone().contiguous().requires_grad_(v.dtype.is_floating_point and "poc" not in k and "aabb" not in k)
          for k, v in net.state_dict().items()}
    cpu_in = [x.clone().requires_grad_(i < 5) for i, x in enumerate(ins)]
    ref = DO.deform_forward(sd, args, *cpu_in, activate=True)
    net = net.to(dev)
    gpu_in = [x.to(dev).requires_grad_(i < 5) for i, x in enumerate(ins)]
    out = fd.deformation.deform(net, *gpu_in[:4], shs=gpu_in[4], time=gpu_in[5], activate=True)
    gen = torch.Generator().manual_seed(5)
    w0, w3 = torch.randn(ref[0].shape, generator=gen), torch.randn(ref[3].shape, generator=gen)
    pn = [k for k in sd if sd[k].requires_grad]
    g_ref = torch.autograd.grad((ref[0] * w0).sum() + (ref[3] * w3).sum(), cpu_in[:5] + [sd[k] for k in pn], allow_unused=True)
    g_gpu = torch.autograd.grad((out[0] * w0.to(dev)).sum() + (out[3] * w3.to(dev)).sum(),
                                gpu_in[:5] + [dict(net.named_parameters())[k] for k in pn], allow_unused=True)
    for k, a, b in zip(["xyz", "scales", "rot", "opacity", "shs"] + pn, g_gpu, g_ref):
        if b is None or float(b.abs().max()) == 0.0:
            assert a is None or float(a.abs().max()) == 0.0, k
        else:
            assert rel_l2(a.cpu().numpy(), b.numpy().reshape(a.shape)) < 1e-4, k
    with torch.no_grad():
        o2 = fd.deformation.deform(net, *gpu_in[:4], shs=gpu_in[4], time=gpu_in[5], activate=True)
    assert o2[0].grad_fn is None
    # the Function object is not reachable without a graph: check through the module-level hook instead
    seen = {}
    orig = fd._lib.lib().fdgs_deform_saved_bytes

    class Spy:
        def __call__(self, *a):
            seen["called"] = True
            return orig(*a)
    fd._lib.lib().fdgs_deform_saved_bytes = Spy()
    try:
        with torch.no_grad():
            fd.deformation.deform(net, *gpu_in[:4], shs=gpu_in[4], time=gpu_in[5], activate=True)
        assert "called" not in seen, "saved-activation buffer sized/allocated under no_grad"
        fd.deformation.deform(net, *gpu_in[:4], shs=gpu_in[4], time=gpu_in[5], activate=True)
        assert seen.get("called"), "grad mode on: the saving forward is expected"
    finally:
        fd._lib.lib().fdgs_deform_saved_bytes = orig
    for a, b in zip(o2, out):
        assert torch.equal(a, b.detach())


def test_aabb_host_copy_is_keyed_on_the_tensor_object_not_its_address():
    """Regression: the host copy of the aabb used to be cached by data_ptr(); the caching allocator hands a freed model's
    aabb address to the next model, which then silently ran with the previous model's bounds."""
    dev = torch.device("cuda:0")
    fd = _fdgs()
    outs = []
    for bounds in ([1.3, 1.25, 1.2], [2.0, 2.5, 3.0]):
        args, net, ins = _net_and_inputs("dynerf_default", 64, 5, dev, safe=False)
        net = net.to(dev)
        net.deformation_net.set_aabb(bounds, [-b for b in bounds])
        gi = [x.to(dev) for x in ins]
        outs.append(fd.deformation.deform(net, gi[0], gi[1], gi[2], gi[3], shs=gi[4], time=0.5, activate=False)[0].cpu())
        del net
        torch.cuda.empty_cache()
    assert float((outs[0] - outs[1]).abs().max()) > 1e-4     # different bounds -> different HexPlane lookups


def test_module_api_matches_reference_signature_and_scalar_time():
    dev = torch.device("cuda:0")
    fd = _fdgs()
    args, net, ins = _net_and_inputs("dnerf_bouncingballs", 300, 5, dev)
    net = net.to(dev)
    gi = [x.to(dev) for x in ins]
    gi[5] = torch.full_like(gi[5], 0.37)
    a = net(gi[0], gi[1], gi[2], gi[3], gi[4], gi[5])
    b = fd.deformation.deform(net, gi[0], gi[1], gi[2], gi[3], shs=gi[4], time=0.37, activate=False)
    c = fd.deformation.deform(net, gi[0], gi[1], gi[2], gi[3], shs_dc=gi[4][:, :1].contiguous(), shs_rest=gi[4][:, 1:].contiguous(),
                              time=0.37, activate=False)
    assert a[4].shape == (300, 16, 3) and a[3].shape == (300, 1)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y.reshape(x.shape)) and torch.equal(x, z.reshape(x.shape))
    # disabled heads (no_do / no_dshs in this config) pass their input through unchanged
    assert torch.equal(a[3], gi[3]) and torch.equal(a[4], gi[4])


def _render_end_to_end_vs_oracle(cfg, stage, active_sh_degree=3, scaling_modifier=1.0, bg=(0.0, 0.0, 0.0), overrides=None, kplanes=None,
                                 n=4000, size=(200, 152)):
    """render() (deform -> activations -> rasterize) against oracle deform -> oracle rasterizer, image and every gradient, at the model's
    active SH degree, a scale modifier and a background colour.  `overrides` / `kplanes` (fields of synthetic.deform_args / entries of its
    kplanes_config): a deformation network of another shape, seeded, perturbed and bounded the way SynthModel does its own."""
    dev = torch.device("cuda:0")
    fd = _fdgs()
    W, H = size
    deformation = None
    if overrides or kplanes:
        torch.manual_seed(21)
        args = synthetic.deform_args(cfg, **(overrides or {}))
        args.kplanes_config.update(kplanes or {})
        deformation = fd.deform_network(args)
        gen = torch.Generator().manual_seed(22)
        with torch.no_grad():
            for name, p in deformation.named_parameters():
                if "grids" in name:
                    p.add_(0.1 * torch.randn(p.shape, generator=gen))
        xyz = synthetic.make_gaussians(n, seed=21)["xyz"]
        deformation.deformation_net.set_aabb(xyz.max(0).values.tolist(), xyz.min(0).values.tolist())
    pc = synthetic.SynthModel(n, cfg, seed=21, deformation=deformation)
    pc.active_sh_degree = active_sh_degree
    cam = synthetic.make_camera(W, H, theta_deg=40.0, time=0.6)
    with torch.no_grad():
        pc._scaling.add_(1.0)  # bigger splats so that most pixels are covered
    sd = {k: v.detach().clone().requires_grad_(v.dtype.is_floating_point and "poc" not in k and "aabb" not in k)
          for k, v in pc._deformation.state_dict().items()}
    leaves = {k: getattr(pc, k).detach().clone().requires_grad_(True) for k in ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest")}
    shs = torch.cat([leaves["_features_dc"], leaves["_features_rest"]], 1)
    if stage == "fine":
        t = torch.full((n, 1), cam.time)
        m3, sc, rot, op, sh = DO.deform_forward(sd, pc._deformation.args, leaves["_xyz"], leaves["_scaling"], leaves["_rotation"],
                                                leaves["_opacity"], shs, t, activate=True)
    else:
        m3, sh = leaves["_xyz"], shs
        sc, op = torch.exp(leaves["_scaling"]), torch.sigmoid(leaves["_opacity"])
        rot = torch.nn.functional.normalize(leaves["_rotation"])
    f = lambda x: np.ascontiguousarray(x.detach().numpy())
    o = RasterOracle(means3D=f(m3), scales=f(sc), rotations=f(rot), opacities=f(op), shs=f(sh), viewmatrix=f(cam.world_view_transform),
                     projmatrix=f(cam.full_proj_transform), campos=f(cam.camera_center), bg=np.array(bg, np.float32), image_height=H,
                     image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), sh_degree=active_sh_degree,
                     scale_modifier=scaling_modifier)
    target = np.random.default_rng(0).random(o.color.shape).astype(np.float32)
    dc = (np.sign(o.color - target) / o.color.size).astype(np.float32)
    go = o.backward(dc)
    # chain the oracle rasterizer gradients through the oracle deformation (autograd on CPU)
    outs = [m3, sc, rot, op, sh]
    gouts = [torch.tensor(go["means3D"]), torch.tensor(go["scales"]), torch.tensor(go["rotations"]),
             torch.tensor(go["opacities"]).reshape(op.shape), torch.tensor(go["shs"]).reshape(sh.shape)]
    wanted = list(leaves.values()) + ([v for v in sd.values() if v.requires_grad] if stage == "fine" else [])
    wnames = list(leaves.keys()) + ([k for k, v in sd.items() if v.requires_grad] if stage == "fine" else [])
    g_ref = torch.autograd.grad(outs, wanted, grad_outputs=gouts, allow_unused=True)

    pc = pc.to(dev)
    pc.active_sh_degree = active_sh_degree
    res = fd.render(cam.to(dev), pc, synthetic.PipelineParams(), torch.tensor(bg, dtype=torch.float32, device=dev), scaling_modifier=scaling_modifier,
                    stage=stage)
    img = res["render"]
    d = np.abs(img.detach().cpu().numpy() - o.color)
    psnr = 10 * math.log10(1.0 / max(float((d ** 2).mean()), 1e-20))
    print(f"[render {cfg} {stage} deg={active_sh_degree} mod={scaling_modifier}] max|dC|={d.max():.2e} mean={d.mean():.2e} psnr={psnr:.1f} dB, visible={(o.radii > 0).sum()}")
    assert d.mean() < 5e-6 and psnr > 75.0
    assert res["depth"].shape == (1, H, W) and res["radii"].shape == (n,) and res["visibility_filter"].dtype == torch.bool
    (img * torch.tensor(dc, device=dev)).sum().backward()
    torch.cuda.synchronize()
    gp = dict(pc.named_parameters())
    rep = {}
    for k, b in zip(wnames, g_ref):
        a = gp[k if k in gp else "_deformation." + k].grad
        if b is None or float(b.abs().max()) == 0.0:
            assert a is None or float(a.abs().max()) < 1e-12, k
            continue
        rep[k] = rel_l2(a.cpu().numpy(), b.numpy().reshape(a.shape))
    worst = sorted(rep.items(), key=lambda kv: -kv[1])[:5]
    print("   worst grad rel-L2: " + ", ".join(f"{k}={v:.2e}" for k, v in worst))
    for k, v in rep.items():
        assert v < 1e-3, (k, v)
    assert rel_l2(res["viewspace_points"].grad.cpu().numpy(), go["means2D"]) < 1e-3
    return gp


@pytest.mark.parametrize("cfg,stage", [("dynerf_default", "fine"), ("dnerf_bouncingballs", "fine"), ("dynerf_default", "coarse")])
def test_render_end_to_end_vs_oracle(cfg, stage):
    _render_end_to_end_vs_oracle(cfg, stage)


@pytest.mark.parametrize("stage,active_sh_degree,scaling_modifier", [("fine", 0, 1.0), ("fine", 1, 1.0), ("fine", 2, 1.0), ("fine", 2, 0.7), ("fine", 3, 0.7),
                                                                     ("coarse", 2, 0.7)])
def test_render_end_to_end_lower_sh_degrees_and_scale_modifier(stage, active_sh_degree, scaling_modifier):
    """The same model, camera and bounds at the SH degrees training passes through (the fused deformation epilogue of the projection backward in
    the fine stage), with a scale modifier and a background whose channels differ.  Coarse stage: the SH bands above the active degree receive
    exactly no gradient."""
    gp = _render_end_to_end_vs_oracle("dynerf_default", stage, active_sh_degree, scaling_modifier, bg=(0.9, 0.1, 0.4))
    if stage == "coarse":
        g = gp["_features_rest"].grad
        assert g is not None and g.shape[1] == 15 and not bool(g[:, (active_sh_degree + 1) ** 2 - 1:].any())


# ---- plane gradients on the matrix cores (D4 splat) -------------------------------------------------------------------
def _plane_grads(cfg, n, order, t, mfma, monkeypatch, seed=13, spread=1.0):
    """d(planes), d(xyz) of sum(out * w) through the HIP backward with one frame time; inputs optionally Hilbert-ordered."""
    dev = torch.device("cuda:0")
    fd = _fdgs()
    set_knob("d4_mfma", "1" if mfma else "0")
    args, net, ins = _net_and_inputs(cfg, n, seed, dev, safe=False, fixed_time=t)
    ins[0] = ins[0] * spread
    if order != "random":
        aabb = net.deformation_net.grid.aabb
        keys = (fd.densify.hilbert_keys if order == "hilbert" else fd.densify.morton_keys)(ins[0], aabb[1], aabb[0])
        perm = torch.argsort(keys)
        ins = [x[perm].contiguous() for x in ins]
    net = net.to(dev)
    gi = [x.to(dev).requires_grad_(i < 5) for i, x in enumerate(ins)]
    out = fd.deformation.deform(net, *gi[:4], shs=gi[4], time=float(t), activate=True)
    ws = [torch.randn(o.shape, generator=torch.Generator().manual_seed(3)).to(dev) for o in out]
    planes = [p for k, p in net.named_parameters() if "grids" in k]
    gr = torch.autograd.grad(sum((o * w).sum() for o, w in zip(out, ws)), [gi[0]] + planes)
    return [g.cpu() for g in gr], (args, net, ins, ws)


@pytest.mark.parametrize("cfg,n,t", [("dynerf_default", 20000, 0.37), ("hypernerf_default", 12000, 1.0), ("dnerf_bouncingballs", 9000, 0.0),
                                     ("dynerf_default", 333, 0.5)])
@pytest.mark.parametrize("order", ["hilbert", "random"])
def test_plane_grad_mfma_splat_equals_per_corner_atomics(cfg, n, t, order, monkeypatch):
    """The matrix-core splat and the per-corner atomic kernel add the same products in a different order: plane and coordinate
    gradients agree to summation noise, on spatially ordered input (everything inside the texel windows) and on random input
    (almost everything outside: the in-kernel fallback)."""
    a, _ = _plane_grads(cfg, n, order, t, True, monkeypatch)
    b, _ = _plane_grads(cfg, n, order, t, False, monkeypatch)
    errs = [rel_l2(x.numpy(), y.numpy()) for x, y in zip(a, b)]
    print(f"[{cfg} n={n} {order}] mfma vs atomics: xyz {errs[0]:.1e}, planes max {max(errs[1:]):.1e}")
    assert errs[0] < 1e-5 and max(errs[1:]) < 2e-5


@pytest.mark.parametrize("cfg,n,t", [("dynerf_default", 20000, 0.37), ("hypernerf_default", 6000, 0.93), ("dnerf_bouncingballs", 5000, 0.2)])
def test_plane_grad_mfma_splat_vs_oracle_on_ordered_input(cfg, n, t, monkeypatch):
    """Hilbert-ordered Gaussians, one frame time: plane + coordinate gradients of the windowed matrix-core splat against the
    CPU oracle (autograd through the explicit-index HexPlane restatement, pinned to the reference modules)."""
    got, (args, net, ins, ws) = _plane_grads(cfg, n, "hilbert", t, True, monkeypatch, spread=0.6)
    risky = DO.discontinuity_margin(net.cpu().state_dict(), args, ins[0], ins[5], parts=True)[0] < 4e-6       # ReLU kinks only: the cells are exact
    sd = {k: v.detach().clone().contiguous().requires_grad_("grids" in k) for k, v in net.state_dict().items()}
    x = ins[0].clone().requires_grad_(True)
    ref = DO.deform_forward(sd, args, x, *ins[1:6], activate=True)
    loss = sum((o * (w.cpu().reshape(o.shape) * (~risky).reshape([-1] + [1] * (o.dim() - 1)))).sum() for o, w in zip(ref, ws))
    g_ref = torch.autograd.grad(loss, [x] + [sd[k] for k in sd if "grids" in k])
    # same masked upstream through the HIP path
    dev = torch.device("cuda:0")
    fd = _fdgs()
    net = net.to(dev)
    gi = [v.to(dev).requires_grad_(i < 5) for i, v in enumerate(ins)]
    out = fd.deformation.deform(net, *gi[:4], shs=gi[4], time=float(t), activate=True)
    m = (~risky).to(dev)
    loss = sum((o * (w * m.reshape([-1] + [1] * (o.dim() - 1)))).sum() for o, w in zip(out, ws))
    g = torch.autograd.grad(loss, [gi[0]] + [p for k, p in net.named_parameters() if "grids" in k])
    errs = [rel_l2(a.cpu().numpy(), b.numpy().reshape(a.shape)) for a, b in zip(g, g_ref)]
    print(f"[{cfg} n={n}] splat vs oracle: xyz {errs[0]:.1e}, planes max {max(errs[1:]):.1e} ({int(risky.sum())} near-ReLU-kink rows masked)")
    assert errs[0] < 1e-3 and max(errs[1:]) < 1e-4


@pytest.mark.parametrize("rows_kb", [0, 20])
def test_plane_grad_mfma_time_rows_that_do_not_fit_lds(rows_kb, monkeypatch):
    """When the private time rows of a level do not fit the workgroup's LDS (large planes, many levels) that level's time planes take
    global atomics in the miss pass: forced here by capping the budget (0 KB: no level fits; 20 KB: level 0 fits, level 1 does not)."""
    set_knob("d4_rows_kb", str(rows_kb))
    a, _ = _plane_grads("dynerf_default", 6000, "hilbert", 0.61, True, monkeypatch)
    set_knob("d4_rows_kb", -1)
    b, _ = _plane_grads("dynerf_default", 6000, "hilbert", 0.61, False, monkeypatch)
    errs = [rel_l2(x.numpy(), y.numpy()) for x, y in zip(a, b)]
    assert errs[0] < 1e-5 and max(errs[1:]) < 2e-5


def test_spatial_order_hint_selects_the_plane_gradient_kernel_not_the_result():
    """The order hint is measured from the positions (once per tensor object) and only chooses between two equivalent kernels."""
    fd = _fdgs()
    dev = torch.device("cuda:0")
    fd.deformation.invalidate_caches()      # (earlier tests leave an answer for fresh [20000,3] tensors behind: the "streak" shortcut)
    g = synthetic.make_gaussians(20000, seed=3)
    x = g["xyz"].to(dev)
    assert fd.deformation.spatial_order_hint(x) is False
    keys = fd.densify.hilbert_keys(x)
    xs = x[torch.argsort(keys)].contiguous()
    assert fd.deformation.spatial_order_hint(xs) is True
    assert fd.deformation.spatial_order_hint(xs[:100].contiguous()) is False        # too few rows to say


@pytest.mark.parametrize("cfg,n,ordered", [("dynerf_default", 9000, True), ("dynerf_default", 9000, False), ("hypernerf_default", 5000, True),
                                           ("dnerf_bouncingballs", 7000, True), ("dynerf_default:L3", 6000, True)])
def test_dead_tile_skipping_is_exact(cfg, n, ordered, monkeypatch):
    """Culled / occluded Gaussians arrive with all-zero gradient rows (gaussian_renderer/__init__.py:134-138: they get no gradient in
    the reference either); in a spatially ordered set they are contiguous, and the backward walks only the 32-row tiles that carry a
    non-zero row (tile_compact_kernel's lists).  With runs of zero upstream rows whose ends are NOT tile-aligned, every gradient must
    equal the FDGS_SKIP_DEAD=0 result (all tiles) up to the re-association of the sums, and fewer tiles must have been processed."""
    dev = torch.device("cuda:0")
    fd = _fdgs()
    # ("dynerf_default:L3": all five heads at net_width 128 with THREE HexPlane levels, C * L = 48 -- the other instance of the
    # weight-stationary backward-data kernel, which no configuration under arguments/ reaches)
    cfg, _, variant = cfg.partition(":")
    args, net, ins = _net_and_inputs(cfg, n, 5, dev, overrides=dict(multires=[1, 2, 4]) if variant == "L3" else None, safe=False, fixed_time=0.43)
    net = net.to(dev)
    mask = torch.ones(n)
    for a, b in ((0, 1000), (1033, 2977), (3100, 3131), (4000, n - 700)):
        mask[a:b] = 0.0
    ws = [torch.randn(s, generator=torch.Generator().manual_seed(2)) for s in ((n, 3), (n, 3), (n, 4), (n, 1), (n, 16, 3))]
    ws = [(w * mask.reshape([-1] + [1] * (w.dim() - 1))).to(dev) for w in ws]
    monkeypatch.setattr(fd.deformation, "COUNT_LIVE_TILES", True)
    res = {}
    # "rows": the default -- on ordered input with saved activations the backward walks the non-zero ROWS (row_compact = 1: row lists, compact
    # gradient rows, activations fetched through the list); "1": the 32-row tile lists (row_compact = 0); "0": every tile
    # "rows2": the row lists built by the two-launch form (tile_compact_kernel + row_gather_kernel: what sets of more than 16 384 tiles take)
    # "rows_d2_32": the row lists walked by the 32-row backward-data kernel (d2_form = 32) where the default is the weight-stationary one
    # (csrc/deform_bwd_ws.h: net_width 128 with all five heads, i.e. the dynerf configuration here)
    for skip in ("rows", "rows_d2_32", "rows2", "1", "0"):
        set_knob("skip_dead", "0" if skip == "0" else "1")
        set_knob("row_compact", {"rows": "1", "rows_d2_32": "1", "rows2": "2"}.get(skip, "0"))
        set_knob("d2_form", "32" if skip == "rows_d2_32" else "0")
        gpu_in = [x.to(dev).requires_grad_(i < 5) for i, x in enumerate(ins)]
        out = fd.deformation.deform(net, *gpu_in[:4], shs=gpu_in[4], time=0.43, activate=True, ordered=ordered)
        params = [(k, p) for k, p in net.named_parameters() if p.requires_grad]
        g = torch.autograd.grad(sum((o * w).sum() for o, w in zip(out, ws)), gpu_in[:5] + [p for _, p in params], allow_unused=True)
        torch.cuda.synchronize()
        res[skip] = (g, fd.deformation.last_live_tiles)
    names = ["xyz", "scales", "rot", "opacity", "shs"] + [k for k, _ in params]
    live, total = res["1"][1][0], res["1"][1][1]
    print(f"[{cfg} n={n} ordered={ordered}] live tiles {live} of {total}; chunks {res['1'][1][2]} of {res['1'][1][3]}; "
          f"row-list units {res['rows'][1][0]}, chunks {res['rows'][1][2]}")
    assert res["0"][1][0] == res["0"][1][1] == total
    expect = len({i // 32 for i in torch.nonzero(mask).squeeze(1).tolist()})
    assert expect <= live <= expect + 3 and live < 0.5 * total
    if ordered:     # the row list: the non-zero rows, padded to whole chunks (128 rows, or the plane-gradient chunk where that is larger)
        nrows = int(mask.sum())
        chunk = max(128, 2048 // args.kplanes_config["output_coordinate_dim"])
        assert res["rows"][1][0] == res["rows2"][1][0] == -(-nrows // chunk) * chunk // 32 and res["rows"][1][0] <= live
    else:           # unordered input keeps the per-corner plane-gradient kernel, which walks Gaussians: tile lists
        assert res["rows"][1][0] == res["rows2"][1][0] == live
    for mode in ("rows", "rows_d2_32", "rows2", "1"):
        worst = {}
        for k, a, b in zip(names, res[mode][0], res["0"][0]):
            if b is None:
                assert a is None
                continue
            worst[k] = rel_l2(a.cpu().numpy(), b.cpu().numpy())
        top = sorted(worst.items(), key=lambda kv: -kv[1])[:3]
        print(f"   skip ({mode}) vs no-skip worst rel-L2: " + ", ".join(f"{k}={v:.2e}" for k, v in top))
        numel = {k: (0 if b is None else b.numel()) for k, b in zip(names, res["0"][0])}
        for k, v in worst.items():
            # a handful of values summed over all Gaussians in a different order (second-layer biases: k <= 48 numbers) carry the
            # re-association noise un-averaged
            # (and the second-layer WEIGHTS, <= 48 x 128 numbers, are sums over every row too: the weight-stationary backward keeps them in registers
            # for a whole launch -- one long float32 chain per element; measured 2.0e-6 on the 128 numbers of the opacity head)
            assert v < (2e-5 if numel[k] <= 64 else 1e-5 if numel[k] <= 48 * 128 else 2e-6), (mode, k, v)
        # rows without an upstream gradient receive exactly the identity-path zeros in every run
        dead = (mask == 0).to(dev)
        for a in res[mode][0][:5]:
            assert float(a[dead].abs().max()) == 0.0


@pytest.mark.parametrize("cfg,n", [("dynerf_default", 9000), ("hypernerf_default", 5000), ("dynerf_default", 40100)])
def test_leftover_tiles_split_by_head_changes_nothing(cfg, n, monkeypatch):
    """D1 deals the tiles left over after the last full round of its persistent loop out BY HEAD (wave u: head u % n_h of tile u / n_h)
    when leftover x heads fits the launch (FDGS_D1_SPLIT=0: every wave takes whole tiles).  Same arithmetic in the same order per
    Gaussian, so outputs, saved activations and therefore gradients must be bit-identical.  9 000 / 5 000 Gaussians: every tile is a
    leftover tile (split active); 40 100: 1 256 tiles = one full round + 232 leftover tiles, which do NOT fit by head (no split)."""
    dev = torch.device("cuda:0")
    fd = _fdgs()
    args, net, ins = _net_and_inputs(cfg, n, 9, dev, safe=False, fixed_time=0.61)
    net = net.to(dev)
    ws = [torch.randn(s, generator=torch.Generator().manual_seed(4)).to(dev) for s in ((n, 3), (n, 3), (n, 4), (n, 1), (n, 16, 3))]
    res = {}
    for split in ("1", "0"):
        set_knob("d1_split", split)
        gpu_in = [x.to(dev).requires_grad_(i < 5) for i, x in enumerate(ins)]
        out = fd.deformation.deform(net, *gpu_in[:4], shs=gpu_in[4], time=0.61, activate=True)
        params = [p for _, p in net.named_parameters() if p.requires_grad]
        g = torch.autograd.grad(sum((o * w).sum() for o, w in zip(out, ws)), gpu_in[:5] + params, allow_unused=True)
        torch.cuda.synchronize()
        res[split] = ([o.detach().clone() for o in out], g)
    for a, b in zip(res["1"][0], res["0"][0]):
        assert torch.equal(a, b)
    for a, b in zip(res["1"][1], res["0"][1]):
        assert (a is None) == (b is None)
        if a is not None:
            # (weight gradients: float atomics in launch order -- two runs of the SAME backward differ by this much; measured up to 1.13e-6 on the
            # second-layer weights, whose elements are sums over every row flushed by 256 workgroups)
            assert torch.equal(a, b) or rel_l2(a.cpu().numpy(), b.cpu().numpy()) < 5e-6
