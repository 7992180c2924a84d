"""The spatial order on the device (csrc/spatial.hip): fdgs_spatial_keys / fdgs_spatial_order against the untouched torch expressions of
fdgs.densify evaluated on the CPU copy of the positions.  Every comparison of keys and permutations is EXACT: the key function is a bit-for-bit
restatement, and LSD radix passes with the row index as payload give THE stable argsort."""
import copy
import ctypes
import importlib

import pytest
import torch

from scenes import rel_l2

pytestmark = pytest.mark.gpu
fdgs = importlib.import_module("4dgaussians_amd")
D = fdgs.densify
synthetic = fdgs.synthetic
SIZES = [1, 63, 64, 65, 4097, 300_000, 1_000_003]
# a box that clamps a large share of N(0, 1.3^2) points; passed as HexPlaneField.aabb is ("max" row first)
AABB_HI, AABB_LO = [1.0, 0.9, 1.1], [-1.0, -1.1, -0.9]


def _points(n, seed=5):
    return torch.randn(n, 3, generator=torch.Generator().manual_seed(seed + n)) * 1.3


def _scratch(n, dev):
    nb = ctypes.c_size_t()
    fdgs._lib.check(fdgs._lib.lib().fdgs_spatial_order_scratch_bytes(n, ctypes.byref(nb)))
    return torch.empty(nb.value, dtype=torch.uint8, device=dev)


def _raw_keys(x, bounds, curve, bits=10):
    n = x.shape[0]
    keys = torch.full((max(n, 1),), -1, dtype=torch.int32, device=x.device)
    scratch = _scratch(n, x.device)
    fdgs._lib.check(fdgs._lib.lib().fdgs_spatial_keys(fdgs._lib.stream_ptr(), n, x.data_ptr(), fdgs._lib.ptr(bounds), fdgs._lib.CURVES[curve], bits,
                                                      scratch.data_ptr(), keys.data_ptr()))
    torch.cuda.synchronize()
    return keys[:n].cpu().long()


def _raw_order(x, bounds, curve, bits=10, want_keys=True):
    n = x.shape[0]
    perm = torch.full((max(n, 1),), -1, dtype=torch.int32, device=x.device)
    skeys = torch.full((max(n, 1),), -1, dtype=torch.int32, device=x.device) if want_keys else None
    scratch = _scratch(n, x.device)
    fdgs._lib.check(fdgs._lib.lib().fdgs_spatial_order(fdgs._lib.stream_ptr(), n, x.data_ptr(), fdgs._lib.ptr(bounds), fdgs._lib.CURVES[curve], bits,
                                                       scratch.data_ptr(), perm.data_ptr(), fdgs._lib.ptr(skeys)))
    torch.cuda.synchronize()
    return perm[:n].cpu().long(), (skeys[:n].cpu().long() if want_keys else None)


def _check(x_cpu, curve, box, bits=10):
    """keys, permutation and sorted keys of the device against the torch functions on the CPU copy."""
    dev = torch.device("cuda:0")
    x = x_cpu.to(dev).contiguous()
    n = x.shape[0]
    keyfn = D.hilbert_keys if curve == "hilbert" else D.morton_keys
    if box:
        ref = keyfn(x.cpu(), AABB_LO, AABB_HI, bits)
        bounds = torch.tensor([AABB_HI, AABB_LO], device=dev)
    else:
        ref = keyfn(x.cpu(), bits=bits)
        bounds = None
    keys = _raw_keys(x, bounds, curve, bits)
    assert torch.equal(keys, ref)
    perm, skeys = _raw_order(x, bounds, curve, bits)
    assert torch.equal(torch.sort(perm).values, torch.arange(n))             # a permutation ...
    assert torch.equal(perm, torch.argsort(ref, stable=True))                # ... THE stable one
    assert torch.equal(skeys, ref[perm])
    perm2, _ = _raw_order(x, bounds, curve, bits, want_keys=False)           # (sorted_keys_opt = NULL)
    assert torch.equal(perm2, perm)
    # the Python host: the same values through fdgs.densify
    lo, hi = (AABB_LO, AABB_HI) if box else (None, None)
    assert D._native(x)
    assert torch.equal(D.spatial_keys(x, lo, hi, curve=curve, bits=bits).cpu(), ref)
    p = D.spatial_order(x, lo, hi, curve=curve, bits=bits)
    assert p.dtype == torch.int32 and p.device == x.device and torch.equal(p.cpu().long(), perm)


@pytest.mark.parametrize("box", [True, False], ids=["aabb", "bbox"])
@pytest.mark.parametrize("curve", ["hilbert", "morton"])
@pytest.mark.parametrize("n", SIZES)
def test_device_keys_and_order_equal_the_torch_functions(n, curve, box):
    _check(_points(n), curve, box)


@pytest.mark.parametrize("curve", ["hilbert", "morton"])
def test_heavy_ties_keep_their_row_order(curve):
    """Every point in one of eight cells: 8 distinct keys over 200 003 rows; the stable argsort is unique, any other valid argsort is not it."""
    n = 200_003
    g = torch.Generator().manual_seed(3)
    corner = torch.randint(0, 2, (n, 3), generator=g).float()
    x = (corner * 2 - 1) * 0.8 + 0.01 * torch.rand(n, 3, generator=g)
    ref = (D.hilbert_keys if curve == "hilbert" else D.morton_keys)(x, [-1.0] * 3, [1.0] * 3, 1)
    assert torch.unique(ref).numel() == 8
    dev = torch.device("cuda:0")
    bounds = torch.tensor([[1.0] * 3, [-1.0] * 3], device=dev)
    for bits in (1, 10):          # one radix pass of 3 bits (8 keys) / four passes over cells that are still only eight clusters
        ref = (D.hilbert_keys if curve == "hilbert" else D.morton_keys)(x, [-1.0] * 3, [1.0] * 3, bits)
        perm, skeys = _raw_order(x.to(dev), bounds, curve, bits)
        assert torch.equal(perm, torch.argsort(ref, stable=True))
        assert torch.equal(skeys, ref[perm])
    # and with exact duplicates of whole rows
    y = x[torch.randint(0, 8, (n,), generator=g)].contiguous()
    _check(y, curve, True)


@pytest.mark.parametrize("box", [True, False], ids=["aabb", "bbox"])
def test_identical_points_give_the_identity(box):
    n = 70_001
    x = torch.full((n, 3), 0.37)
    dev = torch.device("cuda:0")
    perm, skeys = _raw_order(x.to(dev), torch.tensor([AABB_HI, AABB_LO], device=dev) if box else None, "hilbert")
    assert torch.equal(perm, torch.arange(n))
    assert torch.unique(skeys).numel() == 1
    _check(x, "hilbert", box)


@pytest.mark.parametrize("bits", [1, 2, 3, 5, 6, 8, 9])
def test_every_pass_count_lands_in_the_callers_arrays(bits):
    """3 * bits = 3 .. 27 key bits are one to four radix passes: the result must end in `perm` / `sorted_keys_opt` for odd and even counts."""
    _check(_points(20_011), "hilbert", False, bits)
    _check(_points(20_011), "morton", True, bits)


def test_zero_points_are_fine():
    dev = torch.device("cuda:0")
    L = fdgs._lib.lib()
    s = fdgs._lib.stream_ptr()
    assert L.fdgs_spatial_order(s, 0, None, None, 0, 10, None, None, None) == 0
    assert L.fdgs_spatial_keys(s, 0, None, None, 1, 10, None, None) == 0
    e = torch.empty(0, 3, device=dev)
    assert D.spatial_order(e).shape == (0,) and D.spatial_keys(e).shape == (0,)
    torch.cuda.synchronize()


def _model_with_adam_state(n, dev):
    pc = synthetic.SynthModel(n, "dynerf_default", seed=5).to(dev)
    g = torch.Generator().manual_seed(9)
    opt = torch.optim.Adam(pc.optimizer_groups(lr=0.0), lr=0.0, eps=1e-15)
    for grp in opt.param_groups:
        if grp["name"] in D.GROUPS:
            q = grp["params"][0]
            opt.state[q] = {"step": torch.tensor(3.0), "exp_avg": torch.randn(q.shape, generator=g).to(dev),
                            "exp_avg_sq": torch.rand(q.shape, generator=g).to(dev)}
    pc.optimizer = opt
    pc.xyz_gradient_accum, pc.denom = torch.rand(n, 1, generator=g).to(dev), torch.rand(n, 1, generator=g).to(dev)
    pc.max_radii2D, pc._deformation_accum = torch.rand(n, generator=g).to(dev), torch.rand(n, 3, generator=g).to(dev)
    pc._deformation_table = (torch.rand(n, generator=g) < 0.5).to(dev)
    return pc


@pytest.mark.parametrize("curve", ["hilbert", "morton"])
def test_spatial_reorder_is_the_same_with_the_native_order_on_and_off(curve, monkeypatch):
    dev = torch.device("cuda:0")
    n = 50_001
    out = {}
    for native in (True, False):
        monkeypatch.setattr(D, "NATIVE_ORDER", native)
        pc = _model_with_adam_state(n, dev)
        before = pc._xyz.detach().clone()
        perm = D.spatial_reorder(pc, curve=curve)
        assert perm.dtype == torch.int64 and torch.equal(pc._xyz.detach(), before[perm])
        st = {}
        for k, a in D.ATTR.items():
            p = getattr(pc, a)
            assert isinstance(p, torch.nn.Parameter) and p.requires_grad
            grp = [g_ for g_ in pc.optimizer.param_groups if g_["name"] == k][0]
            assert grp["params"][0] is p and float(pc.optimizer.state[p]["step"]) == 3.0
            st[k] = (p.detach(), pc.optimizer.state[p]["exp_avg"], pc.optimizer.state[p]["exp_avg_sq"])
        assert len(pc.optimizer.state) == 6
        side = [getattr(pc, name) for name in ("xyz_gradient_accum", "denom", "max_radii2D", "_deformation_accum", "_deformation_table")]
        out[native] = (perm, st, side)
    (pa, sa, da), (pb, sb, db) = out[True], out[False]
    assert torch.equal(pa, pb)
    for k in sa:
        for x, y in zip(sa[k], sb[k]):
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), k
    for x, y in zip(da, db):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y)
    assert db[4].dtype == torch.bool
    # a given permutation (any integer dtype) moves the same rows through both paths, a model without an optimizer in place
    for native in (True, False):
        monkeypatch.setattr(D, "NATIVE_ORDER", native)
        pc = synthetic.SynthModel(n, "dynerf_default", seed=5).to(dev)
        obj, before = pc._xyz, pc._features_rest.detach().clone()
        D.spatial_reorder(pc, perm=pa.flip(0))
        assert pc._xyz is obj and torch.equal(pc._features_rest.detach(), before[pa.flip(0)])


def test_render_of_an_unordered_model_is_the_same_with_the_native_order_on_and_off(monkeypatch):
    """The permutation is bit-identical, so the frame is: image, depth and radii are compared exactly (the forward has no atomics).  The
    gradients are float atomics in launch order -- two runs of the SAME backward differ --: they are held to 2e-5 rel-L2, the bound
    tests/test_gpu_deform.py uses where equal sums are accumulated in a different order (its loosest one, for the smallest tensors)."""
    dev = torch.device("cuda:0")
    N, W, H = 20_000, 320, 240
    cam = synthetic.orbit_cameras(W, H, n=160)[21].to(dev)
    wimg = torch.randn(3, H, W, generator=torch.Generator().manual_seed(8)).to(dev)
    outs = {}
    for native in (True, False):
        monkeypatch.setattr(D, "NATIVE_ORDER", native)
        fdgs.deformation.invalidate_caches()
        pc = synthetic.SynthModel(N, "dynerf_default", seed=77).to(dev)
        with torch.no_grad():
            pc._scaling.add_(0.5)
        assert fdgs.deformation.spatial_order_hint(pc._xyz) is False
        res = fdgs.render(cam, pc, synthetic.PipelineParams(), torch.zeros(3, device=dev), stage="fine")
        (res["render"] * wimg).sum().backward()
        torch.cuda.synchronize()
        e = fdgs.deformation._perm_cache.get(id(pc._xyz))
        assert e is not None and e[0]() is pc._xyz                     # the frame went through the implicit permutation
        grads = {k: v.grad.clone() for k, v in pc.named_parameters() if v.grad is not None}
        grads["viewspace"] = res["viewspace_points"].grad.clone()
        outs[native] = (res, e[2].clone(), grads)
    (ra, pa, ga), (rb, pb, gb) = outs[True], outs[False]
    assert pa.dtype == pb.dtype == torch.int32 and torch.equal(pa, pb)
    assert torch.equal(ra["render"], rb["render"]) and torch.equal(ra["depth"], rb["depth"]) and torch.equal(ra["radii"], rb["radii"])
    assert torch.equal(ra["visibility_filter"], rb["visibility_filter"])
    assert set(ga) == set(gb)
    worst = {k: (0.0 if torch.equal(ga[k], gb[k]) else rel_l2(gb[k].cpu().numpy(), ga[k].cpu().numpy())) for k in ga}
    print("native vs torch order, gradient rel-L2:", {k: f"{v:.1e}" for k, v in worst.items() if v > 0})
    for k, v in worst.items():
        assert v < 2e-5, (k, v)


def test_implicit_permutation_runs_the_librarys_kernels():
    """After invalidate_caches(), one implicit_permutation of a HIP tensor shows the key kernel and the radix passes in the library's own
    timing report (no torch sort behind it)."""
    dev = torch.device("cuda:0")
    L = fdgs._lib.lib()
    x = torch.nn.Parameter(_points(30_000).to(dev))
    fdgs.deformation.invalidate_caches()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    fdgs._lib.check(L.fdgs_timing_report(buf, len(buf), 1))          # (drop what earlier tests may have left)
    L.fdgs_timing_enable(1)
    try:
        perm = fdgs.deformation.implicit_permutation(x)
        fdgs._lib.check(L.fdgs_timing_report(buf, len(buf), 1))
    finally:
        L.fdgs_timing_enable(0)
    rows = {l.split()[0]: int(l.split()[1]) for l in buf.value.decode().strip().splitlines()}
    assert rows.get("spatial_keys") == 1 and rows.get("spatial_bbox") == 1
    assert rows.get("radix_scatter") == 4 and rows.get("radix_hist") == 4          # 30 key bits: digits of 8, 8, 7, 7
    assert torch.equal(perm.cpu().long(), torch.argsort(D.hilbert_keys(x.detach().cpu()), stable=True))
    assert fdgs.deformation.implicit_permutation(x) is perm                        # cached per tensor object
