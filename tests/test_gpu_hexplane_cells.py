"""GPU tests of the HexPlane index arithmetic (csrc/hexplane_ops.h): the probe fdgs_hexplane_cells equals its host twin bit for bit (the twin
is pinned to F.grid_sample by tests/test_hexplane_cells_host.py), and the PRODUCTION kernels -- forward gather, backward recomputation, both
plane-gradient kernels -- take the fixture's cells on coordinates within 8 float32 ulps of a texel boundary, where a contracted
normalisation (one rounding instead of the reference's two) picks the neighbouring cell."""
import ctypes
import functools
import importlib
import math

import numpy as np
import pytest
import torch

from conftest import set_knob
import hexplane_fixture as HF
from oracle import deform_oracle as DO
from scenes import rel_l2
from test_gpu_deform import _net_and_inputs

pytestmark = pytest.mark.gpu
CANARY_I, CANARY_F, PAD = 0x5A5A5A5A, -7.25, 64


def _fdgs():
    return importlib.import_module("4dgaussians_amd")


@functools.lru_cache(maxsize=None)
def _fixture():
    return HF.load()


def _probe(xyz, t, aabb, time_size):
    """fdgs_hexplane_cells on device copies of the rows; every output buffer sits between PAD canary words that must survive."""
    L = importlib.import_module("4dgaussians_amd._lib")
    dev = torch.device("cuda:0")
    n, nl = xyz.shape[0], len(HF.LEVEL_SIZES)
    dx = torch.from_numpy(xyz).to(dev)
    per_row = isinstance(t, np.ndarray)
    dt = torch.from_numpy(t).to(dev) if per_row else None
    shapes = [((n, nl, 4, 2), torch.int32, CANARY_I), ((n, nl, 4), torch.float32, CANARY_F), ((n, nl, 4), torch.float32, CANARY_F),
              ((n, 4), torch.float32, CANARY_F)]
    bufs = [torch.full((2 * PAD + math.prod(s),), c, dtype=d, device=dev) for s, d, c in shapes]
    p = HF.deform_params(L, dx.data_ptr(), n, aabb, time_size, dt.data_ptr() if per_row else None, 0.0 if per_row else t)
    L.check(L.lib().fdgs_hexplane_cells(L.stream_ptr(), ctypes.byref(p), *[ctypes.c_void_p(b.data_ptr() + 4 * PAD) for b in bufs]))
    torch.cuda.synchronize()
    outs = []
    for b, (s, d, c) in zip(bufs, shapes):
        h = b.cpu()
        assert bool((h[:PAD] == c).all()) and bool((h[-PAD:] == c).all()), "canary words around an output buffer were overwritten"
        outs.append(h[PAD:-PAD].reshape(s).numpy())
    return outs


@pytest.mark.parametrize("per_gaussian_time", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 65, None])
def test_probe_equals_host_twin_bit_for_bit(n, per_gaussian_time):
    """All four outputs, bit for bit: one row, one short of / exactly / one more than a wave, and the whole fixture (both aabbs, both time
    resolutions, about 30 k rows)."""
    fx = _fixture()
    rows = 0
    for aabb_id, aabb in enumerate(HF.AABBS):
        for time_size in (150, 75):
            xyz, t, _ = HF.zip_rows(fx, aabb_id, time_size)
            if n is not None:
                # rows from the middle of the boundary sweep (not only texel 0), odd start
                xyz, t = np.ascontiguousarray(xyz[1001:1001 + n]), np.ascontiguousarray(t[1001:1001 + n])
            tt = t if per_gaussian_time else float(t[len(t) // 3])
            got = _probe(xyz, tt, aabb, time_size)
            want = HF.cells_host(xyz, tt, aabb, time_size)
            for name, a, b in zip(("cells", "w1", "dscale", "q"), got, want):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, aabb_id, time_size, int((a.view(np.uint32) != b.view(np.uint32)).sum()))
            rows += xyz.shape[0]
            if n is not None:
                break
    assert rows >= (25000 if n is None else n)


# ---- the production kernels take the fixture's cells ------------------------------------------------------------------------------------------
N_ROWS, SEED = 4099, 9


@functools.lru_cache(maxsize=None)
def _boundary_inputs(cfg, order, one_time):
    """Model and inputs of test_gpu_deform._net_and_inputs(safe=False) with the xyz rows taken from the fixture: every entry of the model's own
    aabb and level sizes on which the emulated FUSED normalisation flips the cell -- one such coordinate per row, the other two axes random --
    filled to N_ROWS with other entries from the +-8-ulp boundary sweep.  Returns the CPU oracle's results too (computed once, shared by the
    parametrised cases): gradients with the full upstream, the ReLU at-risk set, gradients with the at-risk rows' upstream zeroed."""
    fd = _fdgs()
    fx = _fixture()
    args, net, ins = _net_and_inputs(cfg, N_ROWS, SEED, None, safe=False, fixed_time=0.37 if one_time else None)
    sizes = [64 * m for m in args.multires]
    mine = (fx["aabb_id"] == 0) & (fx["axis"] < 3) & np.isin(fx["size"], sizes)
    flips = np.nonzero(mine & (HF.fused_i0(fx) != fx["i0"]))[0]
    assert 100 <= len(flips) < N_ROWS // 2
    near = (fx["w1"] < 1e-3) | (fx["w1"] > 1.0 - 1e-3)          # within 1e-3 pixel of a boundary: the +-8-ulp sweep (<= 1e-4 pixel at size 256)
    sweep = np.nonzero(mine & near)[0]
    rest = np.setdiff1d(sweep, flips)
    rest = rest[np.random.default_rng(SEED).permutation(len(rest))[:N_ROWS - len(flips)]]
    chosen = np.concatenate([flips, rest])
    assert len(chosen) == N_ROWS
    xyz = ins[0].clone()
    xyz[torch.arange(N_ROWS), torch.from_numpy(fx["axis"][chosen].astype(np.int64))] = torch.from_numpy(fx["x"][chosen].copy())
    ins[0] = xyz
    is_flip = torch.zeros(N_ROWS, dtype=torch.bool)
    is_flip[:len(flips)] = True
    entry = torch.from_numpy(chosen)
    if order == "hilbert":
        aabb = net.deformation_net.grid.aabb
        perm = torch.argsort(fd.densify.hilbert_keys(ins[0], aabb[1], aabb[0]))
    else:
        perm = torch.randperm(N_ROWS, generator=torch.Generator().manual_seed(SEED))
    ins = [x[perm].contiguous() for x in ins]
    is_flip, entry = is_flip[perm], entry[perm].numpy()

    sd = {k: v.detach().clone().contiguous().requires_grad_(v.dtype.is_floating_point and "poc" not in k and "aabb" not in k)
          for k, v in net.state_dict().items()}
    pn = [k for k in sd if sd[k].requires_grad]
    ws = [torch.randn(s, generator=torch.Generator().manual_seed(1)) for s in ((N_ROWS, 3), (N_ROWS, 3), (N_ROWS, 4), (N_ROWS, 1), (N_ROWS, 16, 3))]

    def oracle_grads(mask, decisions=None, only_xyz=False):
        cpu_in = [x.clone().requires_grad_(i < 5) for i, x in enumerate(ins)]
        ref = DO.deform_forward(sd, args, *cpu_in, activate=True, decisions=decisions)
        loss = sum((a * (w * mask.reshape([-1] + [1] * (w.dim() - 1)).to(w.dtype)).reshape(a.shape)).sum() for a, w in zip(ref, ws))
        wanted = cpu_in[:1] if only_xyz else cpu_in[:5] + [sd[k] for k in pn]
        return [r.detach() for r in ref], torch.autograd.grad(loss, wanted, allow_unused=True)

    ones = torch.ones(N_ROWS, dtype=torch.bool)
    ref_out, g_full = oracle_grads(ones)
    # PRECONDITION (CPU only): the test can fail.  Taking the fused arithmetic's cell on the flip rows (KinkDecisions.cell_shift) moves the
    # oracle's own xyz gradient of at least 20 rows by more than 1e-3 of the row scale.
    dec = DO.KinkDecisions(N_ROWS)
    fi0 = HF.fused_i0(fx)
    for r in torch.nonzero(is_flip).squeeze(1).tolist():
        e = entry[r]
        key = (sizes.index(int(fx["size"][e])), int(fx["axis"][e]))
        dec.cell_shift.setdefault(key, torch.zeros(N_ROWS, dtype=torch.int64))[r] = int(fi0[e]) - int(fx["i0"][e])
    _, g_shift = oracle_grads(ones, decisions=dec, only_xyz=True)
    B = g_full[0].numpy()
    scale = np.linalg.norm(B) / math.sqrt(N_ROWS) + 1e-30
    moved = int((np.linalg.norm(g_shift[0].numpy() - B, axis=1) / scale > 1e-3).sum())
    risky = DO.discontinuity_margin(net.state_dict(), args, ins[0], ins[5], parts=True)[0] < 4e-6         # the ReLU part ALONE
    _, g_masked = oracle_grads(~risky)
    return dict(args=args, net=net, ins=ins, ws=ws, pn=pn, ref_out=ref_out, g_full=g_full, g_masked=g_masked, risky=risky, moved=moved,
                n_flips=len(flips), is_flip=is_flip)


@pytest.mark.parametrize("one_time", [False, True], ids=["time_per_gaussian", "one_frame_time"])
@pytest.mark.parametrize("order", ["hilbert", "random"])
@pytest.mark.parametrize("d4_mfma", [1, 0])
@pytest.mark.parametrize("save", [True, False], ids=["saved", "recompute"])
@pytest.mark.parametrize("cfg", ["dynerf_default", "hypernerf_default"])
def test_production_kernels_take_the_fixture_cells(cfg, save, d4_mfma, order, one_time, monkeypatch):
    """Rows that sit within 8 ulps of a texel boundary, among them every fixture entry the fused normalisation gets wrong, through the whole
    HIP deformation forward + backward against the float32 CPU oracle, exactly as test_deform_unfiltered_inputs_flips_counted compares --
    except that the at-risk set is the ReLU margin alone: the distance to a texel boundary excuses no row.
      1. input-gradient rows may differ by more than 1e-3 of the row scale only where the ReLU margin is below 4e-6, and their count is bounded;
      2. with those rows' upstream gradient zeroed every gradient, every plane gradient included, is within 1e-3 rel-L2.
    The value of the interpolant is continuous across a cell boundary; its coordinate derivative and the plane-gradient scatter are not,
    which is what 1. and 2. see.  (With the normalisation contracted to one fma this test fails on the flip rows.)"""
    B = _boundary_inputs(cfg, order, one_time)
    print(f"[{cfg} {order} one_time={one_time}] fused-flip rows {B['n_flips']}, oracle rows moved by their cell shift {B['moved']}, ReLU at-risk {int(B['risky'].sum())}")
    assert B["moved"] >= 20, "precondition: shifting the flip rows' cells must move at least 20 oracle xyz-gradient rows"
    dev = torch.device("cuda:0")
    fd = _fdgs()
    monkeypatch.setattr(fd.deformation, "SAVE_ACTIVATIONS", save)
    set_knob("d4_mfma", d4_mfma)
    n, ins, ws, pn, risky = N_ROWS, B["ins"], B["ws"], B["pn"], B["risky"].numpy()
    bound = max(8, int(4e-5 * n * (1 + 5) * 128))
    assert risky.sum() <= bound, f"{risky.sum()} at-risk rows of {n}"
    net = B["net"].to(dev)
    names = ["xyz", "scales", "rot", "opacity", "shs"] + pn

    def hip_grads(mask):
        gpu_in = [x.to(dev).requires_grad_(i < 5) for i, x in enumerate(ins)]
        out = fd.deformation.deform(net, *gpu_in[:4], shs=gpu_in[4], time=0.37 if one_time else gpu_in[5], activate=True, ordered=order == "hilbert")
        loss = sum((a * (w * mask.reshape([-1] + [1] * (w.dim() - 1)).to(w.dtype)).to(dev).reshape(a.shape)).sum() for a, w in zip(out, ws))
        g = torch.autograd.grad(loss, gpu_in[:5] + [dict(net.named_parameters())[k] for k in pn], allow_unused=True)
        return out, g

    out, g_gpu = hip_grads(torch.ones(n, dtype=torch.bool))
    for a, b in zip(out, B["ref_out"]):
        assert rel_l2(a.detach().cpu().numpy(), b.numpy().reshape(a.shape)) < 2e-5
    flipped = np.zeros(n, bool)
    for k, a, b in zip(names[:5], g_gpu[:5], B["g_full"][:5]):
        A, Bm = a.cpu().numpy().reshape(n, -1), b.numpy().reshape(n, -1)
        scale = np.linalg.norm(Bm) / math.sqrt(n) + 1e-30
        rowerr = np.linalg.norm(A - Bm, axis=1) / scale
        flipped |= rowerr > 1e-3
        if k == "xyz":
            bad = np.nonzero((rowerr > 1e-3) & ~risky)[0]
            if len(bad):
                print(f"   xyz rows that differ without a ReLU kink: {len(bad)} ({int(B['is_flip'].numpy()[bad].sum())} of them fused-flip rows); "
                      f"worst {bad[np.argsort(-rowerr[bad])][:5].tolist()} -> {np.round(np.sort(rowerr[bad])[::-1][:5], 4).tolist()}")
    print(f"   rows whose input gradient differs {int(flipped.sum())} (bound {bound})")
    assert not np.any(flipped & ~risky), f"{int((flipped & ~risky).sum())} rows differ without being near a ReLU kink"
    assert flipped.sum() <= bound
    _, g_gpu = hip_grads(torch.tensor(~risky))
    worst = {}
    for k, a, b in zip(names, g_gpu, B["g_masked"]):
        if b is not None:
            worst[k] = rel_l2(a.cpu().numpy(), b.numpy().reshape(a.shape))
    print("   masked-upstream worst rel-L2: " + ", ".join(f"{k}={v:.2e}" for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:3]))
    for k, v in worst.items():
        assert v < 1e-3, (k, v)
