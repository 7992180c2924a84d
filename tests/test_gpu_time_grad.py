"""dL/dt on the device: the kernels of csrc/deform_time_grad.h against their host twin on the kernel's own input, fdgs.deform's time gradient
against the float64 oracle, render()'s routes against each other, and a time fitted through them.  Run with -m gpu on MI355X.

1. Kernel against twin.  The real fdgs.deform forward and backward run with random upstream weights and a time leaf; behind the backward
   the probe fdgs_deform_time_grad_dfeat copies DFEAT out of the scratch (Gaussian order, a live byte per row) and the host twin
   fdgs_deform_time_grad_host evaluates the same rows in double.  Bounds, from the reduction shape (u = 2^-23):
     per row    |device - twin| <= (A + 2) u sum|addend|_row,  A = 6 L C addends per row (level, time plane, x-corner, channel): every
                addend is a product of float32 factors that are themselves a few roundings from the twin's (far fewer than A), a lane adds
                its 3 L addends in order and an xor butterfly of log2(2 C) steps adds the lanes -- depth < A;
     scalar     |device - twin| <= (A + 2 + D) u sum|addend| over all live rows, D = 256 / G + G + 1 with G = 4 * 64 / (2 C) lane groups per
                workgroup: a group adds its 256 / G rows in order, one thread adds the G group sums, and the last stage adds the workgroups'
                partials in double and rounds once.
   Neither bound is measured.  Shapes: N = 1, 31, 257, 1531; 5 000 rows with row_compact 0, 1, 2 (tile lists, both ways of building the row
   list) and about half the 32-row tiles without upstream gradient, the backward's scratch pre-filled with NaN (dead tiles, pad entries and
   garbage DFEAT rows all occur: asserted through fdgs_deform_bwd_live_tiles); SAVE_ACTIVATIONS off; ordered and unordered; C = 16 / 32,
   L = 2 / 3, three and five heads.  Two runs on one scratch are bit-equal.  Every gradient the backward produced is bit-equal with and
   without the time leaf: in every case above the whole gradient arena is compared (torch.equal) before and after the two launches, which
   run behind the backward and write nothing into it; across two separate backwards the per-Gaussian gradients are torch.equal, while the
   plane and weight gradients -- float atomics in launch order, two runs of the SAME backward differ in their last bits -- are held to the
   5e-6 that tests/test_gpu_deform.py::test_leftover_tiles_split_by_head_changes_nothing allows two such runs.
2. Against the oracle: T.grad in both modes, activate on and off, against float64 autograd through deform_forward on rows that are safe in
   ReLU, spatial cell AND time row (time_grad_common.safe_inputs): rel-L2 < 1e-4, the bound _parity holds every other gradient to.
   The scalar is held to the same 1e-4 of the same norm: |device - sum_n ref_n| < 1e-4 |ref|_2.  The rows carry random signs and their sum
   cancels (|sum| / |ref|_2 = 0.025, 0.29, 1.35, 1.45 over the four cases, from the float64 oracle on the CPU), so an error measured against
   |sum| is the rows' error times that cancellation: the oracle's OWN float32 evaluation is 4.4e-5 of |sum| from its float64 one in the
   first case (dynerf, t = 0.37, activate off; 8e-7 .. 5e-6 in the others) with rows that agree to 6e-6, and the device, whose rows agree to
   6e-6 too, read 1.01e-4 of |sum| there (2.6e-6 of |ref|_2) -- a first version of this test divided by |sum| and failed on that one case.
3. render(): fused against two-node with a time leaf (2e-5, as for the camera leaves), the model's gradients with against without it
   (2e-5), and time + camera leaves + alpha in one frame against the separate frames.

Measured on MI355X: device against twin, worst |difference| / bound 0.004 per row and 0.001 for the scalar, over every case; T.grad per row
against the float64 oracle 6.2e-6 .. 9.1e-6; the scalar 2.6e-6, 4.6e-7, 1.6e-6, 8.0e-6 of |ref|_2; render() dL/dt fused against two-node
1.1e-7 and 0; the model's gradients with against without the time leaf <= 7.4e-7; the joint frame against the separate frames: time
1.1e-7, camera 1.5e-7, model 4.8e-7; dL/dt through the implicit permutation against without it 6.8e-6.
"""
import importlib

import numpy as np
import pytest
import torch

from conftest import set_knob
from oracle import deform_oracle as DO
import time_grad_common as TC

pytestmark = pytest.mark.gpu
U = 2.0 ** -23


def _mod():
    return importlib.import_module("4dgaussians_amd")


def _bounds(net):
    grid = net.deformation_net.grid
    C, L = grid.grid_config[0]["output_coordinate_dim"], len(grid.grids)
    A = 6 * L * C
    G = 4 * (64 // (2 * C))
    return A, 256 // G + G + 1


def _run(net, ins, time, mask=None, ordered=None, activate=True, leaf=True, poison=False, monkeypatch=None):
    """fdgs.deform forward + backward of sum(out * w) on the device (w seeded; rows with mask == 0 get zero upstream gradient).  With a time
    leaf the probe and a second fdgs_deform_time_grad run behind the backward.  -> dict(grads, t_grad, dfeat, live, again, tiles)."""
    fd = _mod()
    D, lib = fd.deformation, fd._lib
    dev = torch.device("cuda:0")
    got = {}
    orig_tg, orig_prep = D.time_gradient, D.backward_prepare

    def time_gradient(st, b):
        before = b.arena.clone()                      # every gradient that fdgs_deform_bwd has just produced
        out = orig_tg(st, b)
        got["again"] = orig_tg(st, b)                 # (the same backward's scratch, read twice)
        got["arena_untouched"] = torch.equal(b.arena, before)
        N, F = st.p.N, st.p.C * st.p.L
        got["dfeat"] = torch.full((N, F), float("nan"), device=dev)
        got["live"] = torch.full((N,), 7, dtype=torch.uint8, device=dev)
        lib.check(lib.lib().fdgs_deform_time_grad_dfeat(lib.stream_ptr(), st.p, b.g, lib.ptr(got["dfeat"]), lib.ptr(got["live"])))
        tiles = (lib.c_uint32 * 4)()
        lib.check(lib.lib().fdgs_deform_bwd_live_tiles(lib.stream_ptr(), st.p, b.g.scratch, tiles))
        got["tiles"] = tuple(int(x) for x in tiles)
        return out

    def backward_prepare(*a, **k):
        b = orig_prep(*a, **k)
        if poison:       # what the kernels do not write stays NaN: a dead tile's DFEAT rows, the entries behind a list's end
            b.scratch[:b.scratch.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
        return b

    monkeypatch.setattr(D, "time_gradient", time_gradient)
    monkeypatch.setattr(D, "backward_prepare", backward_prepare)
    gpu_in = [x.to(dev).requires_grad_(True) for x in ins[:5]]
    if isinstance(time, torch.Tensor):
        T = time.to(dev).requires_grad_(leaf)
    else:
        T = torch.tensor(float(time), device=dev, requires_grad=True) if leaf else float(time)
    out = D.deform(net, *gpu_in[:4], shs=gpu_in[4], time=T, activate=activate, ordered=ordered)
    gen = torch.Generator().manual_seed(11)
    ws = [torch.randn(o.shape, generator=gen) for o in out]
    if mask is not None:
        ws = [w * mask.reshape([-1] + [1] * (w.dim() - 1)).to(w.dtype) for w in ws]
    params = [p for p in net.parameters() if p.requires_grad]
    wanted = gpu_in + params + ([T] if leaf else [])
    grads = torch.autograd.grad(sum((o * w.to(dev)).sum() for o, w in zip(out, ws)), wanted, allow_unused=True)
    torch.cuda.synchronize()
    got["grads"] = grads[:len(gpu_in) + len(params)]
    got["t_grad"] = grads[-1] if leaf else None
    got["ws"] = ws
    return got


def _against_twin(net_cpu, ins, time, got, tag):
    """The device's T.grad against the host twin on the probe's DFEAT, inside the bounds of the module docstring."""
    A, depth = _bounds(net_cpu)
    dfeat, live = got["dfeat"].cpu().numpy(), got["live"].cpu().numpy()
    assert set(np.unique(live)) <= {0, 1} and np.isfinite(dfeat).all() and not dfeat[live == 0].any()
    p, keep = TC.host_params(net_cpu, ins[0], time)
    rows, tot, arows, atot = TC.host_twin(p, dfeat, live)
    dev_t = got["t_grad"].detach().cpu().double().numpy().reshape(-1)
    assert torch.equal(got["again"].reshape(-1), got["t_grad"].reshape(-1).float()), "two runs on one scratch differ"
    assert got["arena_untouched"], "fdgs_deform_time_grad changed a gradient the backward had produced"
    if isinstance(time, torch.Tensor):
        err, bound = np.abs(dev_t - rows), (A + 2) * U * arows
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"[{tag}] per row: worst |device - twin| / bound {worst:.3f} (A = {A}); live rows {int(live.sum())} of {live.size}")
        assert np.all(err <= bound), (tag, int(np.argmax(err - bound)))
        assert not dev_t[live == 0].any()
        cl = TC.clamped(time).numpy()
        assert not dev_t[cl].any()                                       # t = 1.0, t = 1.2: exactly 0
        assert np.count_nonzero(dev_t[(live == 1) & ~cl]) > 0.5 * ((live == 1) & ~cl).sum()      # (tile form: a live tile's rows without a gradient give 0)
    else:
        err, bound = abs(dev_t[0] - tot), (A + 2 + depth) * U * atot
        print(f"[{tag}] scalar: device {dev_t[0]:.6e} twin {tot:.6e} |diff| / bound {err / max(bound, 1e-300):.3f} (A = {A}, depth {depth}); "
              f"live rows {int(live.sum())} of {live.size}")
        assert err <= bound, (tag, err, bound)
        if float(time) >= 1.0:
            assert dev_t[0] == 0.0
        else:
            assert atot > 0 and tot != 0.0 and dev_t[0] != 0.0
    return rows, tot


SHAPES = [("dynerf_default", 1), ("dnerf_bouncingballs", 31), ("hypernerf_default", 257), ("dynerf_default", 1531)]


@pytest.mark.parametrize("cfg,n", SHAPES)
@pytest.mark.parametrize("mode", ["rows", "scalar"])
def test_kernel_against_twin(cfg, n, mode, monkeypatch):
    args, net, ins = TC.candidates(cfg, max(n, 8))
    if n == 1:
        ins = [x[4:5].contiguous() for x in ins]              # (a row with a random time)
    time = ins[5] if mode == "rows" else 0.37
    got = _run(net.to("cuda:0"), ins, time, monkeypatch=monkeypatch)
    _against_twin(net.cpu(), ins, time, got, f"{cfg} n={n} {mode}")


def _half_dead_mask(n):
    """Upstream gradient only for the 32-row tiles 0, 3 (mod 4), and there not for every fifth row: dead tiles, and a row list that needs padding."""
    r = torch.arange(n)
    tile = r // 32
    return (((tile % 4 == 0) | (tile % 4 == 3)) & (r % 5 != 0)).float()


@pytest.mark.parametrize("cfg", ["dynerf_default", "dnerf_bouncingballs"])         # (the weight-stationary D2 and the 32-row D2 with row lists)
@pytest.mark.parametrize("row_compact", [0, 1, 2])
def test_kernel_against_twin_on_lists_with_dead_tiles(cfg, row_compact, monkeypatch):
    n = 5000
    args, net, ins = TC.candidates(cfg, n)
    mask = _half_dead_mask(n)
    set_knob("row_compact", row_compact)
    got = _run(net.to("cuda:0"), ins, 0.37, mask=mask, ordered=True, poison=True, monkeypatch=monkeypatch)
    live_units, tiles = got["tiles"][0], got["tiles"][1]
    assert tiles == (n + 127) // 128 * 4 and 0 < live_units < tiles, got["tiles"]           # dead tiles occur
    live = got["live"].cpu().numpy()
    if row_compact:
        assert np.array_equal(live, (mask.numpy() != 0).astype(np.uint8))                   # the row list: exactly the rows with a gradient
        assert live_units * 32 > int(live.sum()) and (live_units * 32) % 128 == 0           # ... padded: pad entries occur
    else:
        tile_live = (mask.reshape(-1)[: n // 32 * 32].reshape(-1, 32).sum(1) != 0).numpy()
        assert np.array_equal(live[: n // 32 * 32].reshape(-1, 32).max(1) != 0, tile_live) and not live.reshape(-1)[32:96].any()
    _against_twin(net.cpu(), ins, 0.37, got, f"{cfg} n={n} row_compact={row_compact}")


@pytest.mark.parametrize("mode", ["rows", "scalar"])
def test_kernel_against_twin_per_gaussian_times_with_dead_tiles_and_unordered_scalar(mode, monkeypatch):
    """The tile form: per-Gaussian times (always), and one frame time on unordered input (per-corner D4)."""
    n = 5000
    args, net, ins = TC.candidates("hypernerf_default", n)
    time = ins[5] if mode == "rows" else 0.61
    got = _run(net.to("cuda:0"), ins, time, mask=_half_dead_mask(n), ordered=False, poison=True, monkeypatch=monkeypatch)
    assert 0 < got["tiles"][0] < got["tiles"][1]
    _against_twin(net.cpu(), ins, time, got, f"hypernerf n={n} tile form {mode}")


@pytest.mark.parametrize("mode", ["rows", "scalar"])
def test_kernel_against_twin_on_the_recompute_path(mode, monkeypatch):
    monkeypatch.setattr(_mod().deformation, "SAVE_ACTIVATIONS", False)
    args, net, ins = TC.candidates("dynerf_default", 1531)
    time = ins[5] if mode == "rows" else 0.37
    got = _run(net.to("cuda:0"), ins, time, ordered=True, monkeypatch=monkeypatch)
    _against_twin(net.cpu(), ins, time, got, f"dynerf n=1531 recompute {mode}")


@pytest.mark.parametrize("t", [1.0, 1.2])
def test_a_clamped_frame_time_gives_exactly_zero(t, monkeypatch):
    args, net, ins = TC.candidates("dynerf_default", 700)
    got = _run(net.to("cuda:0"), ins, t, ordered=True, monkeypatch=monkeypatch)
    assert got["t_grad"].shape == () and float(got["t_grad"]) == 0.0


@pytest.mark.parametrize("mode,ordered", [("rows", None), ("scalar", True), ("scalar", False)])
def test_the_backwards_own_gradients_are_bit_equal_with_and_without_the_time_leaf(mode, ordered, monkeypatch):
    args, net, ins = TC.candidates("dynerf_default", 2100)
    net = net.to("cuda:0")
    time = ins[5] if mode == "rows" else 0.37
    a = _run(net, ins, time, mask=_half_dead_mask(2100), ordered=ordered, monkeypatch=monkeypatch)
    monkeypatch.undo()
    b = _run(net, ins, time, mask=_half_dead_mask(2100), ordered=ordered, leaf=False, monkeypatch=monkeypatch)
    assert a["t_grad"] is not None and a["arena_untouched"] and b["t_grad"] is None and len(a["grads"]) == len(b["grads"])
    # (the plane and weight gradients are float atomics in launch order: two runs of the SAME backward differ in their last bits, see the
    # module docstring; within one run the arena is bit-equal before and after the time-gradient launches: _against_twin)
    for i, (x, y) in enumerate(zip(a["grads"], b["grads"])):
        assert (x is None) == (y is None)
        if x is None:
            continue
        if i < 5:
            assert torch.equal(x, y), i
        else:
            assert torch.equal(x, y) or TC.rel_l2(x.cpu().numpy(), y.cpu().numpy()) < 5e-6, i


# ---- 2. against the oracle --------------------------------------------------------------------------------------------------------------

def _oracle_time_grad(args, net, ins, t, ws, activate):
    """d sum(out * w) / dt per row, float64 autograd through oracle.deform_oracle.deform_forward."""
    dt = torch.float64
    sd = {k: (v.detach().to(dt) if v.dtype.is_floating_point else v) for k, v in net.state_dict().items()}
    tt = t.detach().reshape(-1, 1).to(dt).requires_grad_(True)
    out = DO.deform_forward(sd, args, *[x.detach().to(dt) for x in ins[:5]], tt, activate=activate)
    g, = torch.autograd.grad(sum((o * w.to(dt).reshape(o.shape)).sum() for o, w in zip(out, ws)), tt)
    return g.reshape(-1).numpy()


@pytest.mark.parametrize("cfg,n", TC.ORACLE_CASES)
@pytest.mark.parametrize("activate", [False, True])
def test_per_gaussian_time_gradient_against_the_float64_oracle(cfg, n, activate, monkeypatch):
    args, net, ins = TC.safe_inputs(cfg, n)
    got = _run(net.to("cuda:0"), ins, ins[5], activate=activate, monkeypatch=monkeypatch)
    ref = _oracle_time_grad(args, net.cpu(), ins, ins[5], got["ws"], activate)
    dev_t = got["t_grad"].cpu().double().numpy().reshape(-1)
    assert got["t_grad"].shape == (n, 1)
    cl = TC.clamped(ins[5]).numpy()
    assert np.linalg.norm(ref) > 0 and np.count_nonzero(ref[~cl]) == (~cl).sum() and not ref[cl].any() and not dev_t[cl].any()
    e = TC.rel_l2(dev_t, ref)
    print(f"[{cfg} n={n} act={activate}] T.grad per row vs float64 oracle: rel-L2 {e:.2e}; |ref| {np.linalg.norm(ref):.3e}")
    assert e < 1e-4


@pytest.mark.parametrize("cfg,n,t", TC.ORACLE_SCALAR_CASES)
@pytest.mark.parametrize("activate", [False, True])
def test_scalar_time_gradient_against_the_float64_oracle(cfg, n, t, activate, monkeypatch):
    args, net, ins = TC.safe_inputs_one_time(cfg, n, t)
    got = _run(net.to("cuda:0"), ins, t, activate=activate, monkeypatch=monkeypatch)
    ref = _oracle_time_grad(args, net.cpu(), ins, ins[5], got["ws"], activate)
    dev_t = float(got["t_grad"])
    e = abs(dev_t - ref.sum()) / np.linalg.norm(ref)
    print(f"[{cfg} n={n} t={t} act={activate}] scalar T.grad {dev_t:.6e} vs float64 sum {ref.sum():.6e}: |diff| / |rows|_2 {e:.2e} "
          f"(/ |sum| {abs(dev_t - ref.sum()) / abs(ref.sum()):.2e}); |rows|_2 {np.linalg.norm(ref):.3e}")
    assert got["t_grad"].shape == () and abs(ref.sum()) > 1e-3 * np.abs(ref).sum() / np.sqrt(n)
    assert e < 1e-4


# ---- 3. render() ----------------------------------------------------------------------------------------------------------------------

class _Pipe:
    convert_SHs_python = compute_cov3D_python = debug = False


class _AlphaPipe(_Pipe):
    render_alpha = True


W_, H_, N_ = 128, 96, 2000


def _render_run(cfg, monkeypatch, fused=True, time_leaf=True, cam_leaves=False, alpha=False, override=False):
    fd = _mod()
    syn = fd.synthetic
    dev = torch.device("cuda:0")
    monkeypatch.setattr(fd.renderer, "FUSED_BACKWARD", fused)
    gen = torch.Generator().manual_seed(4)
    w, wd, wa = (torch.randn(c, H_, W_, generator=gen).to(dev) for c in (3, 1, 1))
    pc = syn.SynthModel(N_, cfg, seed=23)
    with torch.no_grad():
        pc._scaling.add_(1.0)
    pc = pc.to(dev)
    cam = syn.make_camera(W_, H_, theta_deg=-35.0, time=0.45).to(dev)
    if cam_leaves:
        for k in ("world_view_transform", "full_proj_transform", "camera_center"):
            setattr(cam, k, getattr(cam, k).clone().requires_grad_(True))
    T = None
    if time_leaf:
        T = torch.tensor(0.45, device=dev, requires_grad=True)
        cam.time = T
    oc = torch.rand(N_, 3, generator=gen).to(dev) if override else None
    res = fd.render(cam, pc, _AlphaPipe() if alpha else _Pipe(), torch.zeros(3, device=dev), stage="fine", override_color=oc)
    loss = (res["render"] * w).sum() + (res["depth"] * wd).sum()
    if alpha:
        loss = loss + (res["alpha"] * wa).sum()
    loss.backward()
    torch.cuda.synchronize()
    cg = {k: getattr(cam, k).grad for k in ("world_view_transform", "full_proj_transform", "camera_center")}
    return res, {k: p.grad.clone() for k, p in pc.named_parameters() if p.grad is not None}, cg, (None if T is None else T.grad)


@pytest.mark.parametrize("cfg", ["dynerf_default", "dnerf_bouncingballs"])
def test_render_fused_against_two_node_with_a_time_leaf(cfg, monkeypatch):
    ra, ga, _, ta = _render_run(cfg, monkeypatch, fused=True)
    rb, gb, _, tb = _render_run(cfg, monkeypatch, fused=False)
    r0, g0, _, t0 = _render_run(cfg, monkeypatch, fused=True, time_leaf=False)
    rc, gc, _, tc = _render_run(cfg, monkeypatch, fused=True, override=True)
    assert type(ra["render"].grad_fn).__name__ == "_FusedRenderTimeFunctionBackward" and t0 is None
    assert type(r0["render"].grad_fn).__name__ == "_FusedRenderFunctionBackward"
    assert torch.equal(ra["render"], rb["render"]) and torch.equal(ra["render"], r0["render"]) and torch.equal(ra["depth"], r0["depth"])
    assert ta.shape == () and tb.shape == () and float(ta.abs()) > 0 and tc.shape == () and float(tc.abs()) > 0
    e_time = abs(float(ta) - float(tb)) / abs(float(tb))
    worst_model = max((TC.rel_l2(ga[k].cpu().numpy(), g0[k].cpu().numpy()), k) for k in ga)
    worst_two = max((TC.rel_l2(gb[k].cpu().numpy(), g0[k].cpu().numpy()), k) for k in gb)
    print(f"[{cfg}] dL/dt fused {float(ta):.6e} two-node {float(tb):.6e}: rel {e_time:.1e}; model gradients with vs without the time leaf: fused "
          f"{worst_model[0]:.1e} ({worst_model[1]}), two-node {worst_two[0]:.1e} ({worst_two[1]})")
    assert set(ga) == set(g0) == set(gb)
    assert e_time < 2e-5 and worst_model[0] < 2e-5 and worst_two[0] < 2e-5


def test_render_time_and_camera_leaves_and_alpha_in_one_frame(monkeypatch):
    cfg = "dynerf_default"
    r_all, g_all, c_all, t_all = _render_run(cfg, monkeypatch, cam_leaves=True, alpha=True)
    r_t, g_t, _, t_only = _render_run(cfg, monkeypatch, alpha=True)
    r_c, g_c, c_only, _ = _render_run(cfg, monkeypatch, time_leaf=False, cam_leaves=True, alpha=True)
    assert type(r_all["render"].grad_fn).__name__ == "_FusedRenderTimeFunctionBackward"
    assert type(r_c["render"].grad_fn).__name__ == "_FusedRenderCameraFunctionBackward"
    assert torch.equal(r_all["render"], r_t["render"]) and torch.equal(r_all["alpha"], r_c["alpha"])
    e_time = abs(float(t_all) - float(t_only)) / abs(float(t_only))
    worst_cam = max((TC.rel_l2(c_all[k].cpu().numpy(), c_only[k].cpu().numpy()), k) for k in c_all)
    worst_model = max((TC.rel_l2(g_all[k].cpu().numpy(), g_c[k].cpu().numpy()), k) for k in g_all)
    print(f"joint frame: dL/dt vs the time-only frame rel {e_time:.1e}; camera gradients vs the camera-only frame {worst_cam[0]:.1e} ({worst_cam[1]}); "
          f"model gradients {worst_model[0]:.1e} ({worst_model[1]})")
    assert all(v is not None and float(v.abs().sum()) > 0 for v in c_all.values()) and float(t_all.abs()) > 0
    assert e_time < 2e-5 and worst_cam[0] < 2e-5 and worst_model[0] < 2e-5


def test_render_scalar_time_gradient_does_not_depend_on_the_row_order(monkeypatch):
    """The implicit Hilbert permutation (models of IMPLICIT_ORDER_MIN_N rows and more whose rows are in no order) reorders the rows the
    kernels see; dL/dt is a sum over them."""
    fd = _mod()
    syn = fd.synthetic
    dev = torch.device("cuda:0")
    n = fd.renderer.IMPLICIT_ORDER_MIN_N + 300
    gen = torch.Generator().manual_seed(4)
    w = torch.randn(3, H_, W_, generator=gen).to(dev)

    def run(implicit):
        monkeypatch.setattr(fd.renderer, "IMPLICIT_ORDER", implicit)
        pc = syn.SynthModel(n, "dynerf_default", seed=23)
        with torch.no_grad():
            pc._scaling.add_(0.5)
        pc = pc.to(dev)
        cam = syn.make_camera(W_, H_, theta_deg=-35.0, time=0.45).to(dev)
        cam.time = torch.tensor(0.45, device=dev, requires_grad=True)
        res = fd.render(cam, pc, _Pipe(), torch.zeros(3, device=dev), stage="fine")
        (res["render"] * w).sum().backward()
        return float(cam.time.grad), pc._xyz.grad.clone()

    (ta, xa), (tb, xb) = run(True), run(False)
    e = abs(ta - tb) / abs(tb)
    print(f"dL/dt through the implicit permutation {ta:.6e}, without {tb:.6e}: rel {e:.1e}")
    assert tb != 0.0 and e < 2e-5 and TC.rel_l2(xa.cpu().numpy(), xb.cpu().numpy()) < 2e-5
