"""The deformation backward at short and ragged live-row lists.  Run with -m gpu on MI355X; the first test needs no GPU.

With one frame time on spatially ordered rows the backward walks a list of the rows that carry an upstream gradient, padded to whole units
of 128 entries (csrc/deform_bwd_lists.h).  The rest of the suite reaches that machinery with a few thousand live rows in long runs, and
compares it with the oracle only when every row is live.  Here the list is empty, one row long, ends in the last (partial) tile, holds
exactly 127 / 128 / 129 entries, has one live row per tile, or is so short that most workgroups of the matrix-core splat get an
all-padding or empty share (masks and expected counts: tests/live_rows_common.py, checked on the CPU by the first test).

1. Oracle leg (n = 300 and 31, safe rows, activate on, ordered, a float time: the row form, asserted through the live-tile counter):
   forward rel-L2 < 2e-5; every gradient of the masked sum against the CPU oracle's autograd rel-L2 < 1e-4; tensors the oracle has as
   exactly zero are exactly zero (or None) on the device; per-Gaussian gradients of rows with mask 0 are exactly 0.0.
2. Form leg (HIP against HIP, n = 300 and 4 100, the three configurations and dynerf with three HexPlane levels): row lists built in one
   launch and in two, the 32-row backward-data kernel on the row list, tile lists, the per-corner plane-gradient kernel, the recompute
   path and the all-tiles reference (skip_dead 0).  Every mode equals the reference within the bounds of
   test_gpu_deform.py::test_dead_tile_skipping_is_exact (2e-5 / 1e-5 / 2e-6 by element count), is finite, gives exact zeros on rows
   with mask 0 (everything exactly zero under `none`), reports the expected number of 32-row units, and two runs of one mode give
   bit-equal per-Gaussian gradients.  The rows are safe rows here as well: with a one-row list a single ReLU decision that the
   recompute path rounds the other way would be the whole gradient.
3. dL/dt at the same edges (time_grad_common.safe_inputs_one_time, the one-frame-time form of safe_inputs -- the row form needs one
   frame time; a time leaf, n = 300, row and tile lists): against float64 autograd through the oracle within 1e-4 of the reference rows'
   2-norm, exactly 0 under `none`; the gradient arena is torch.equal before and after fdgs_deform_time_grad; two reads of one scratch
   are equal.
4. The rasterizer's epilogue as the producer of the flags: a SynthModel of 256 rows -- deformation.spatial_order_hint measures nothing
   below 256 rows, and the Hilbert-ordered cube of 256 measures 0.096 against its threshold of 0.1 -- rendered by a camera turned away
   from the set (nothing visible: every gradient exactly zero, no unit walked) and by one turned 45 degrees to the side (65 rows
   visible: one 128-entry unit, gradients equal the skip_dead 0 run within 2e-6).

Stale scratch.  In legs 1 - 3 every backward's scratch starts as a copy of the bytes a finished backward of the `all` mask at the same
shape left behind (itself run on a zero-filled scratch with the two-launch row form, which writes every list), never as what the
allocator returns: every stale flag, list entry and counter is a valid value of another frame, so a kernel that reads behind its list's
end computes a wrong number that the comparisons catch and never forms a wild address.  Nothing here fills a scratch with NaN.

Not tested at its own size: the automatic switch to the two-launch form above 16 384 tiles (524 288 rows); row_compact 2 forces that
form here.

No defect was found in the kernels or the host code: every case passed as first written, except that a first version drew the upstream
weights from N(0, 1) and one bias gradient (three numbers, the plain column sum of those weights) cancelled to 1 / 1 600 of its terms on
the `even` rows of 4 100, where the two-launch row form read 2.2e-5 against the 2e-5 bound -- the inputs' conditioning, see _weights.

Live rows of every case: LR.LIVE_ROWS (n = 31: 0, 1, 1, 16, 31; n = 300: 0, 1, 1, 1, 12, 127, 128, 129, 10, 10, 150, 300, 75;
n = 4 100: 0, 1, 1, 1, 4, 127, 128, 129, 129, 125, 2 050, 4 100, 1 025, in the order of LR.MASKS).  No bound here is derived from the
oracle's float32 / float64 distance: the one-row cases meet 1e-4 as they are.

Measured on MI355X (worst over the masks and sizes of a configuration):
  oracle leg, forward / gradients against 2e-5 / 1e-4: dynerf 9.2e-8 / 9.8e-7 (xyz, n = 300 `last`), hypernerf 7.8e-8 / 5.3e-7 (xyz,
    n = 31 `last`), dnerf 8.0e-8 / 6.5e-7 (xyz, n = 300 `last`);
  form leg, worst rel-L2 as a fraction of its bound, row forms / tile forms: dynerf 0.31 (plane (0, 3) of level 0 6.2e-7, n = 300
    `mid`) / 0.21; hypernerf 0.58 (plane (2, 3) of level 0 1.2e-6, n = 4 100 `last`) / 0.41; dnerf 0.19 / 0.16; dynerf with three
    levels 0.29 / 0.25 -- the largest are one-row lists, where the matrix-core splat's window sums and the all-tiles run differ
    un-averaged;
  dL/dt against 1e-4 of |rows|_2: dynerf 2.0e-5 (`last`, tile lists), hypernerf 4.7e-5 (`first`, row list), dnerf 3.9e-5 (`last`, row
    list): one-row lists, where the scalar is that row's own cancelling sum of 6 L C addends;
  epilogue: 65 rows visible from the side camera, one unit of 128 entries against 8 tiles; row form against all tiles 6.6e-7 (_xyz),
    viewspace 4.9e-8; the mirrored camera: 0 visible, 0 units, every gradient exactly zero.
The module's 195 GPU tests take 26 s together.
What notices a wrong kernel, tried on two development builds: the row-list kernels without the zero fill of the compact rows behind the
list's end (the stale rows of the `all` frame stay) failed 119 of the 195; the splat's share cut one entry short (`tot - 1`) failed
exactly the eleven `pad` cases of legs 1 and 2, the lists whose 128th entry is live.
"""
import copy
import importlib

import numpy as np
import pytest
import torch

from conftest import set_knob
from oracle import deform_oracle as DO
from scenes import rel_l2
import live_rows_common as LR
import time_grad_common as TC
from test_gpu_deform import _net_and_inputs
from test_gpu_time_grad import _oracle_time_grad, _run as _time_run

gpu = pytest.mark.gpu
synthetic = importlib.import_module("4dgaussians_amd.synthetic")

ORACLE_CFGS = [("dynerf_default", 0.37), ("hypernerf_default", 1.0), ("dnerf_bouncingballs", 0.0)]
FORM_CFGS = ORACLE_CFGS + [("dynerf_default:L3", 0.37)]        # (":L3": multires [1, 2, 4] -- the other instance of the weight-stationary D2)
TIME_CFGS = [("dynerf_default", 0.37), ("hypernerf_default", 0.37), ("dnerf_bouncingballs", 0.613)]
TIME_MASKS = ("none", "first", "last", "pad", "pad+1", "stride32")


def _fdgs():
    return importlib.import_module("4dgaussians_amd")


# ---- the masks, on the CPU ---------------------------------------------------------------------------------------------------------------

def test_masks_hold_the_rows_they_are_documented_to_hold():
    """Every (mask, n) of the GPU tests: live rows (pinned in LR.LIVE_ROWS), distinct live 32-row tiles and the padded row-list length,
    recomputed here by other means than LR.expected."""
    assert sorted(LR.LIVE_ROWS) == sorted(LR.SIZES)
    for n in LR.SIZES:
        assert n % 32 != 0 and sorted(LR.LIVE_ROWS[n]) == sorted(LR.masks_for(n))
    for n, name in LR.cases():
        m = LR.row_mask(name, n)
        per = LR.output_masks(name, n)
        assert m.shape == (n,) and len(per) == 5 and all(q.shape == (n,) and set(q.unique().tolist()) <= {0.0, 1.0} for q in per + [m])
        assert torch.equal(torch.stack(per).amax(0), m)                       # a row is live when any output gives it a gradient
        rows = [i for i in range(n) if m[i] != 0]
        live, tiles, padded = LR.expected(name, n)
        assert live == len(rows) == LR.LIVE_ROWS[n][name], (name, n, live)
        assert tiles == len({i // 32 for i in rows}) and padded == (live + 127) // 128 * 128 and padded % 128 == 0
        assert (padded == 0) == (name == "none") and 0 <= padded - live < 128
        # the masked upstream weights cannot cancel in a column sum (see _weights): positive on the rows of their mask, zero elsewhere
        for q, w in zip(per, _masked(_weights(n), per)):
            w = w.reshape(n, -1)
            assert bool((w[q != 0] >= 0.5).all()) and not bool(w[q == 0].any())
    assert LR.tiles_total(31) == 4 and LR.tiles_total(300) == 12 and LR.tiles_total(4100) == 132
    for n in (300, 4100):
        last_tile = n // 32
        assert LR.expected("none", n) == (0, 0, 0) and LR.expected("first", n) == (1, 1, 128) and LR.expected("mid", n) == (1, 1, 128)
        assert LR.row_mask("mid", n)[45] == 1 and LR.row_mask("last", n)[n - 1] == 1 and (n - 1) // 32 == last_tile
        tail = torch.nonzero(LR.row_mask("tail_tile", n)).squeeze(1)
        assert int(tail.min()) == last_tile * 32 and int(tail.max()) == n - 1 and LR.expected("tail_tile", n)[1] == 1
        assert LR.expected("all", n)[1] == last_tile + 1 == LR.expected("stride32", n)[1] == LR.expected("stride32", n)[0]
        assert LR.expected("stride33", n)[1] == LR.expected("stride33", n)[0]      # one row per tile, the live lane walks
        assert {int(i) % 32 for i in torch.nonzero(LR.row_mask("stride33", n)).squeeze(1)} == set(range(min(32, -(-n // 33))))
        for name, k in (("pad-1", 127), ("pad", 128), ("pad+1", 129)):
            r = torch.nonzero(LR.row_mask(name, n)).squeeze(1)
            assert r.numel() == k and int((r[1:] - r[:-1]).max()) > 1 and LR.expected(name, n)[2] == (128 if k <= 128 else 256)
        per = dict(zip(LR.OUTPUTS, LR.output_masks("one_output", n)))
        assert not per["scales"].any() and all(per[o].sum() >= 16 for o in LR.ONE_OUTPUT_GROUPS)
        assert float(sum(per.values()).max()) == 1.0 and abs(LR.expected("one_output", n)[0] - n / 4) < 1     # disjoint groups, a quarter of the rows
    assert LR.expected("stride32", 4100)[2] == 256 and LR.expected("stride32", 300)[2] == 128


# ---- shared device-side helpers ----------------------------------------------------------------------------------------------------------

_inputs_cache, _oracle_cache, _image_cache = {}, {}, {}


def _inputs(cfg, n, t):
    """(args, network, n safe rows at the frame time t), made once per (cfg, n) and read-only afterwards."""
    key = (cfg, n)
    if key not in _inputs_cache:
        name, _, variant = cfg.partition(":")
        _inputs_cache[key] = _net_and_inputs(name, n, 3, None, overrides=dict(multires=[1, 2, 4]) if variant == "L3" else None, safe=True,
                                             fixed_time=t, candidates=4 * n + 256)
    return _inputs_cache[key]


class _StaleScratch:
    """Wraps deformation.backward_prepare: every new scratch is filled with `image` (the bytes a finished backward left behind), or with
    zeros while there is no image; `last` is the latest call's buffers."""

    def __init__(self, monkeypatch):
        D = _fdgs().deformation
        orig = D.backward_prepare
        self.image, self.last = None, None

        def backward_prepare(*a, **k):
            b = orig(*a, **k)
            if self.image is None:
                b.scratch.zero_()
            else:
                assert b.scratch.numel() == self.image.numel(), "the stale image is of another shape"
                b.scratch.copy_(self.image)
            self.last = b
            return b

        monkeypatch.setattr(D, "backward_prepare", backward_prepare)


MODE_DEFAULTS = dict(skip_dead=1, row_compact=1, d2_form=0, d4_mfma=-1, save=True)
MODES = {            # name -> (knobs that differ from the defaults, which list the backward walks)
    "rows": (dict(), "rows"),
    "rows2": (dict(row_compact=2), "rows"),
    "rows_d2_32": (dict(d2_form=32), "rows"),
    "tiles": (dict(row_compact=0), "tiles"),
    "d4_atomics": (dict(d4_mfma=0), "tiles"),             # (the per-corner kernel walks Gaussians: tile lists)
    "recompute": (dict(save=False), "tiles"),             # (the row form fetches saved activations through the list)
    "all_tiles": (dict(skip_dead=0), "all"),
}


def _set_mode(monkeypatch, mode):
    k = dict(MODE_DEFAULTS, **MODES[mode][0])
    for name in ("skip_dead", "row_compact", "d2_form", "d4_mfma"):
        set_knob(name, k[name])
    monkeypatch.setattr(_fdgs().deformation, "SAVE_ACTIVATIONS", k["save"])


def _weights(n):
    """Upstream weights 0.5 + |N(0, 1)|: positive on purpose.  A second-layer bias gradient is the plain column sum of these weights over
    the live rows (times a positive Jacobian for scales and opacity), and a sum of signed weights is a random walk that may cancel --
    N(0, 1) from this seed on the `even` rows of 4 100 sums to |s| = 1.05 out of sum|x| = 1 650 per column, and the float32 summation
    noise of either form (0.2 u sum|x|) then read 2.2e-5 of |s|; the single opacity column cancels to 1 / 114 on the four rows of
    `tail_tile` even around a mean of 0.5.  A relative bound on such a sum measures the inputs' cancellation, not the kernels.  With
    positive weights sum|x| / |s| = 1 in every case (held by the first test)."""
    gen = torch.Generator().manual_seed(11)
    return [0.5 + torch.randn(s, generator=gen).abs() for s in ((n, 3), (n, 3), (n, 4), (n, 1), (n, 16, 3))]


def _masked(ws, per):
    return [w * m.reshape([-1] + [1] * (w.dim() - 1)) for w, m in zip(ws, per)]


def _device_run(net, ins, t, ws):
    """deform() forward and the backward of sum(out * w) on the device -> (outputs, names, gradients, last_live_tiles)."""
    dev = torch.device("cuda:0")
    D = _fdgs().deformation
    gpu_in = [x.to(dev).requires_grad_(i < 5) for i, x in enumerate(ins)]
    out = D.deform(net, *gpu_in[:4], shs=gpu_in[4], time=float(t), activate=True, ordered=True)
    params = [(k, p) for k, p in net.named_parameters() if p.requires_grad]
    D.last_live_tiles = None
    g = torch.autograd.grad(sum((o * w.to(dev).reshape(o.shape)).sum() for o, w in zip(out, ws)), gpu_in[:5] + [p for _, p in params],
                            allow_unused=True)
    torch.cuda.synchronize()
    return [o.detach() for o in out], list(LR.OUTPUTS) + [k for k, _ in params], g, D.last_live_tiles


def _prepare(cfg, n, t, monkeypatch):
    """Network on the device, safe rows, and a scratch hook that holds the stale image of this shape."""
    args, net, ins = _inputs(cfg, n, t)
    net = net.to("cuda:0")
    monkeypatch.setattr(_fdgs().deformation, "COUNT_LIVE_TILES", True)
    hook = _StaleScratch(monkeypatch)
    key = ("deform", cfg, n)
    if key not in _image_cache:
        _set_mode(monkeypatch, "rows2")
        _, _, _, tiles = _device_run(net, ins, t, _weights(n))
        assert tiles[0] == -(-n // 128) * 4, tiles           # every row listed
        _image_cache[key] = hook.last.scratch.clone()
    hook.image = _image_cache[key]
    return args, net, ins, hook


def _check_units(name, n, form, tiles):
    """last_live_tiles[0] against the numbers of the CPU test: a case cannot silently run another path."""
    live, live_tiles, padded = LR.expected(name, n)
    assert tiles is not None and tiles[1] == LR.tiles_total(n), tiles
    if form == "rows":
        assert tiles[0] == padded // 32, (name, n, form, tiles)
    elif form == "tiles":
        assert live_tiles <= tiles[0] <= live_tiles + 3, (name, n, form, tiles)
    else:
        assert tiles[0] == tiles[1], (name, n, form, tiles)


def _dead_rows_exactly_zero(name, n, grads):
    dead = (LR.row_mask(name, n) == 0).to("cuda:0")
    if bool(dead.any()):
        for k, a in zip(LR.OUTPUTS, grads[:5]):
            assert float(a[dead].abs().max()) == 0.0, k


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------------------

def _oracle(cfg, n, t):
    """The CPU oracle's outputs on the safe rows, with their graph: made once per (cfg, n); each mask takes its gradients from it."""
    key = (cfg, n)
    if key not in _oracle_cache:
        args, net, ins = _inputs(cfg, n, t)
        sd = {k: v.detach().cpu().clone().contiguous().requires_grad_(v.dtype.is_floating_point and "poc" not in k and "aabb" not in k)
              for k, v in net.state_dict().items()}
        cpu_in = [x.clone().requires_grad_(i < 5) for i, x in enumerate(ins)]
        ref = DO.deform_forward(sd, args, *cpu_in, activate=True)
        pnames = [k for k in sd if sd[k].requires_grad]
        _oracle_cache[key] = dict(ref=ref, wanted=cpu_in[:5] + [sd[k] for k in pnames], pnames=pnames)
    return _oracle_cache[key]


@gpu
@pytest.mark.parametrize("n,mask", LR.cases((300, 31)))
@pytest.mark.parametrize("cfg,t", ORACLE_CFGS)
def test_row_form_against_the_oracle(cfg, t, n, mask, monkeypatch):
    args, net, ins, hook = _prepare(cfg, n, t, monkeypatch)
    o = _oracle(cfg, n, t)
    ws = _masked(_weights(n), LR.output_masks(mask, n))
    g_ref = torch.autograd.grad(sum((a * w.reshape(a.shape)).sum() for a, w in zip(o["ref"], ws)), o["wanted"], allow_unused=True,
                                retain_graph=True)
    _set_mode(monkeypatch, "rows")
    out, names, g, tiles = _device_run(net, ins, t, ws)
    _check_units(mask, n, "rows", tiles)
    fwd = {k: rel_l2(a.cpu().numpy(), b.detach().numpy().reshape(a.shape)) for k, a, b in zip(LR.OUTPUTS, out, o["ref"])}
    assert max(fwd.values()) < 2e-5, fwd
    assert names == list(LR.OUTPUTS) + o["pnames"]
    report, zeros = {}, 0
    for k, a, b in zip(names, g, g_ref):
        if b is None or not bool(b.any()):
            assert a is None or not bool(a.any()), (k, "the oracle has exactly zero here")
            zeros += 1
            continue
        assert a is not None and bool(torch.isfinite(a).all()), k
        report[k] = rel_l2(a.cpu().numpy(), b.numpy().reshape(a.shape))
    worst = sorted(report.items(), key=lambda kv: -kv[1])[:3]
    print(f"[oracle {cfg} n={n} {mask}] live rows {LR.expected(mask, n)[0]}, units {tiles[0]}; forward {max(fwd.values()):.1e}; {zeros} tensors exactly "
          f"zero; worst grad rel-L2: " + ", ".join(f"{k}={v:.2e}" for k, v in worst))
    if mask == "none":
        assert not report
    _dead_rows_exactly_zero(mask, n, g)
    for k, v in report.items():
        assert v < 1e-4, (k, v)


# ---- 2. the forms against each other -------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("n,mask", LR.cases((300, 4100)))
@pytest.mark.parametrize("cfg,t", FORM_CFGS)
def test_every_form_equals_the_all_tiles_backward(cfg, t, n, mask, monkeypatch):
    args, net, ins, hook = _prepare(cfg, n, t, monkeypatch)
    ws = _masked(_weights(n), LR.output_masks(mask, n))
    res = {}
    for mode, (_, form) in MODES.items():
        _set_mode(monkeypatch, mode)
        _, names, g, tiles = _device_run(net, ins, t, ws)
        _, _, g2, tiles2 = _device_run(net, ins, t, ws)
        _check_units(mask, n, form, tiles)
        assert tiles2 == tiles
        for k, a, b in zip(names[:5], g[:5], g2[:5]):
            assert torch.equal(a, b), (mode, k, "two runs of one mode differ")
        res[mode] = g
    ref = res["all_tiles"]
    worst_all = {}
    for mode in MODES:
        worst = {}
        for k, a, b in zip(names, res[mode], ref):
            assert (a is None) == (b is None), (mode, k)
            if b is None:
                continue
            assert bool(torch.isfinite(a).all()), (mode, k)
            if mask == "none" or not bool(b.any()):
                assert not bool(a.any()), (mode, k, "exactly zero in the all-tiles run")
                continue
            if mode == "all_tiles":
                continue
            worst[k] = rel_l2(a.cpu().numpy(), b.cpu().numpy())
            # (the bounds of test_dead_tile_skipping_is_exact: a handful of numbers summed over every row carry the re-association un-averaged)
            bound = 2e-5 if b.numel() <= 64 else 1e-5 if b.numel() <= 48 * 128 else 2e-6
            worst_all[mode] = max(worst_all.get(mode, (0.0, "", 0.0)), (worst[k] / bound, k, worst[k]))
        _dead_rows_exactly_zero(mask, n, res[mode])
    print(f"[forms {cfg} n={n} {mask}] live rows {LR.expected(mask, n)[0]}; worst rel-L2 / bound per mode: "
          + ", ".join(f"{m}={v[0]:.2f} ({v[1]} {v[2]:.1e})" for m, v in worst_all.items()))
    for m, v in worst_all.items():
        assert v[0] < 1.0, (m, v)


# ---- 3. dL/dt at the same edges ----------------------------------------------------------------------------------------------------------

_time_inputs_cache = {}


@gpu
@pytest.mark.parametrize("row_compact", [1, 0])
@pytest.mark.parametrize("mask", TIME_MASKS)
@pytest.mark.parametrize("cfg,t", TIME_CFGS)
def test_scalar_time_gradient_at_short_lists(cfg, t, mask, row_compact, monkeypatch):
    n = 300
    if cfg not in _time_inputs_cache:
        args, net, ins = TC.safe_inputs_one_time(cfg, n, t)
        _time_inputs_cache[cfg] = (args, net, copy.deepcopy(net).to("cuda:0"), ins)
    args, net_cpu, net, ins = _time_inputs_cache[cfg]
    monkeypatch.setattr(_fdgs().deformation, "COUNT_LIVE_TILES", True)
    hook = _StaleScratch(monkeypatch)          # (installed first: test_gpu_time_grad._run wraps it with its own hooks)
    key = ("time", cfg, n)
    if key not in _image_cache:
        _set_mode(monkeypatch, "rows2")
        _, _, _, tiles = _device_run(net, ins, t, _weights(n))
        assert tiles[0] == -(-n // 128) * 4, tiles
        _image_cache[key] = hook.last.scratch.clone()
    hook.image = _image_cache[key]
    _set_mode(monkeypatch, "rows" if row_compact else "tiles")
    m = LR.row_mask(mask, n)
    got = _time_run(net, ins, t, mask=m, ordered=True, monkeypatch=monkeypatch)
    live, live_tiles, padded = LR.expected(mask, n)
    if row_compact:
        assert got["tiles"][0] == padded // 32, got["tiles"]
        assert np.array_equal(got["live"].cpu().numpy(), (m.numpy() != 0).astype(np.uint8))       # the list: exactly the rows with a gradient
    else:
        assert live_tiles <= got["tiles"][0] <= live_tiles + 3, got["tiles"]
    assert got["t_grad"].shape == () and got["arena_untouched"], "fdgs_deform_time_grad changed a gradient the backward had produced"
    assert torch.equal(got["again"].reshape(-1), got["t_grad"].reshape(-1).float()), "two reads of one scratch differ"
    dev_t = float(got["t_grad"])
    if mask == "none":
        assert dev_t == 0.0
        return
    ref = _oracle_time_grad(args, net_cpu, ins, ins[5], got["ws"], True)
    assert np.count_nonzero(ref) == live and not ref[m.numpy() == 0].any()
    e = abs(dev_t - ref.sum()) / np.linalg.norm(ref)
    print(f"[time {cfg} t={t} {mask} row_compact={row_compact}] live rows {live}; dL/dt {dev_t:.6e} vs float64 {ref.sum():.6e}: |diff| / |rows|_2 {e:.2e}")
    assert np.isfinite(dev_t) and e < 1e-4


# ---- 4. the rasterizer's epilogue as producer --------------------------------------------------------------------------------------------

SEC5_N = 256             # deformation.spatial_order_hint: no answer below 256 rows; the reordered cube of 256 measures 0.096 < 0.1
SEC5_VISIBLE = 65        # rows with radii > 0 from the camera turned 45 degrees (pinned: a change to the scene cannot move the case)


class _Pipe:
    convert_SHs_python = compute_cov3D_python = debug = False


def _turned(cam, yaw_deg):
    """`cam` turned about its own vertical axis: 180 degrees mirror it (the whole set is behind it), 45 leave one edge of the set in view."""
    c, s = np.cos(np.radians(yaw_deg)), np.sin(np.radians(yaw_deg))
    turn = torch.tensor([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], dtype=torch.float32)
    proj = torch.tensor(synthetic.projection_matrix(cam.znear, cam.zfar, cam.FoVx, cam.FoVy)).transpose(0, 1)      # (as make_camera builds it)
    wvt = (cam.world_view_transform @ turn).contiguous()
    return synthetic.SynthCamera(cam.image_width, cam.image_height, cam.FoVx, cam.FoVy, wvt, (wvt @ proj).contiguous(), cam.camera_center, cam.time)


def _render_grads(pc, cam, w):
    fd = _fdgs()
    dev = torch.device("cuda:0")
    for p in pc.parameters():
        p.grad = None
    fd.deformation.last_live_tiles = None
    res = fd.render(cam, pc, _Pipe(), torch.tensor([0.1, 0.2, 0.3], device=dev), stage="fine")
    (res["render"] * w).sum().backward()
    torch.cuda.synchronize()
    return res, {k: p.grad.clone() for k, p in pc.named_parameters() if p.grad is not None}, res["viewspace_points"].grad.clone(), \
        fd.deformation.last_live_tiles


@gpu
def test_short_lists_from_the_rasterizers_epilogue(monkeypatch):
    fd = _fdgs()
    dev = torch.device("cuda:0")
    pc = synthetic.SynthModel(SEC5_N, "dynerf_default", seed=23)
    with torch.no_grad():
        pc._scaling.add_(0.5)
    fd.densify.spatial_reorder(pc)
    pc = pc.to(dev)
    assert fd.deformation.spatial_order_hint(pc._xyz) is True
    base = synthetic.make_camera(128, 96, theta_deg=20.0, time=0.6)
    w = torch.randn(3, 96, 128, generator=torch.Generator().manual_seed(4)).to(dev)
    monkeypatch.setattr(fd.deformation, "COUNT_LIVE_TILES", True)
    total = SEC5_N // 32
    # (b) first: it shows which parameters receive a gradient at all
    side = _turned(base, 45.0).to(dev)
    runs = {}
    for skip in ("1", "0"):
        set_knob("skip_dead", skip)
        runs[skip] = _render_grads(pc, side, w)
    visible = int((runs["1"][0]["radii"] > 0).sum())
    print(f"[epilogue n={SEC5_N}] side camera: visible {visible}, units {runs['1'][3]}, all-tiles run {runs['0'][3]}")
    assert visible == SEC5_VISIBLE and 0 < visible < 128
    assert runs["1"][3][0] == 4 and runs["0"][3][0] == runs["0"][3][1] == total          # one 128-entry unit; every tile
    assert torch.equal(runs["1"][0]["render"], runs["0"][0]["render"]) and set(runs["1"][1]) == set(runs["0"][1])
    worst = max((rel_l2(runs["1"][1][k].cpu().numpy(), runs["0"][1][k].cpu().numpy()), k) for k in runs["0"][1])
    vs = rel_l2(runs["1"][2].cpu().numpy(), runs["0"][2].cpu().numpy())
    print(f"   row form vs all tiles: worst {worst[0]:.1e} ({worst[1]}), viewspace {vs:.1e}")
    assert all(bool(torch.isfinite(v).all()) for v in runs["1"][1].values()) and float(runs["1"][1]["_xyz"].abs().max()) > 0
    assert worst[0] < 2e-6 and vs < 2e-6
    # (a) the mirrored camera: nothing in front of it
    set_knob("skip_dead", "1")
    res, grads, vsg, tiles = _render_grads(pc, _turned(base, 180.0).to(dev), w)
    assert int((res["radii"] > 0).sum()) == 0 and tiles is not None and tiles[0] == 0 and tiles[1] == total, tiles
    assert set(grads) == set(runs["1"][1])
    for k, v in grads.items():
        assert bool(torch.isfinite(v).all()) and not bool(v.any()), k
    assert bool(torch.isfinite(vsg).all()) and not bool(vsg.any())
