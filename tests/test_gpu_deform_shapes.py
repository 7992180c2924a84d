"""The fused HIP deformation at EVERY compiled (net_width, C * L) instance and every head set, against the CPU oracle (pinned to the
reference's modules at two of these shapes too: tests/test_oracle_deform.py).

tests/test_gpu_deform.py runs the three named configs: four of the ten instances of dispatch_wf (csrc/deform.hip) and two of the 32 head
masks.  Here: net_width {64, 128} x (C, levels) so that C * L takes all of {32, 48, 64, 96, 128} with both C wherever it can be formed two
ways; masks 31 and 7 on every shape, all 32 masks on two shapes; every forward form forced, with the form that really ran read from the
library's own timing rows; the one-frame-time backward (row lists, matrix-core splat) with the weight-stationary and the 32-row
backward-data kernel and with the per-corner plane-gradient kernel; the recompute backward; render() end to end at two head sets the
rasterizer's fused epilogue had not seen; and the shape that passes validation without a compiled instance.

Bounds: the project's own (test_gpu_deform._parity: outputs rel-L2 < 2e-5, every gradient on safe rows < 1e-4; test_dead_tile_skipping_is_exact
for two HIP runs that differ by the order of their sums).  Sizes: 300 rows (no multiple of 16, 32 or 128: 19 sixteen-row tiles, three
128-row pads), 31 (one partial tile) and 1531 on 13 workgroups (persistent loop with leftover tiles) at C * L = 128; planes of base
resolution [16, 16, 16, 10].

What these tests found: at net_width 64 with C * L = 96 or 128 (the reference's argument defaults among them) the gradient of the trunk
weight was wrong by a rel-L2 of 2.4 - 3.3 in every leg: the weight-gradient kernel's LDS accumulator held W * W floats, its rows are
32 * ceil(C * L / 32) floats wide (csrc/deform_wgrad.h, fixed with these tests).  Every other tensor agreed at every shape.

Measured on the MI355X (worst rel-L2 over the tensors of a leg, against the oracle; "forms": the forward form observed at d1_form =
0 / 8 / 16 / 32; leg 2: as planned / d2_form 32 / d4_mfma 0, in brackets the first two against each other; leg 4: worst of the three
forced forms).  Bounds: forward < 2e-5, every gradient < 1e-4, bracket < 2e-5 / 1e-5 / 2e-6 by tensor size.

  net_width, C x L    mask     n  forms        forward  leg 1    leg 2                                  leg 3    leg 4
   64, 16 x 2 =  32     31   300  16/8/16/32   8.8e-08  6.6e-07  5.4e-07 / 5.3e-07 / 5.4e-07 (1.3e-07)  6.4e-07  6.6e-07
   64, 16 x 2 =  32      7   300  16/8/16/32   8.8e-08  5.4e-07  4.9e-07 / 4.8e-07 / 5.0e-07 (1.3e-07)  5.1e-07  5.6e-07
   64, 32 x 1 =  32     31   300  16/8/16/32   8.5e-08  6.0e-07  5.4e-07 / 5.4e-07 / 5.4e-07 (1.8e-07)  5.2e-07  6.2e-07
   64, 32 x 1 =  32      7   300  16/8/16/32   8.3e-08  3.8e-07  5.2e-07 / 5.3e-07 / 5.1e-07 (8.4e-08)  4.0e-07  4.0e-07
   64, 16 x 3 =  48     31   300  16/8/16/32   8.7e-08  5.1e-07  9.0e-07 / 9.0e-07 / 8.9e-07 (1.8e-07)  5.7e-07  5.6e-07
   64, 16 x 3 =  48      7   300  16/8/16/32   7.8e-08  6.9e-07  4.6e-07 / 4.5e-07 / 4.5e-07 (9.0e-08)  6.6e-07  6.7e-07
   64, 32 x 2 =  64     31   300  16/8/16/32   8.7e-08  5.7e-07  5.8e-07 / 5.8e-07 / 5.8e-07 (1.4e-07)  5.3e-07  6.8e-07
   64, 32 x 2 =  64      7   300  16/8/16/32   8.5e-08  8.1e-07  5.3e-07 / 5.3e-07 / 5.4e-07 (1.0e-07)  9.1e-07  9.0e-07
   64, 16 x 4 =  64     31   300  16/8/16/32   8.6e-08  5.0e-07  1.1e-06 / 1.1e-06 / 1.2e-06 (3.6e-07)  5.2e-07  5.2e-07
   64, 16 x 4 =  64      7   300  16/8/16/32   7.9e-08  5.3e-07  5.0e-07 / 4.9e-07 / 5.0e-07 (9.3e-08)  5.9e-07  6.0e-07
   64, 32 x 3 =  96     31   300  16/8/16/32   8.8e-08  5.3e-07  7.0e-07 / 7.0e-07 / 7.0e-07 (1.2e-07)  5.3e-07  5.7e-07
   64, 32 x 3 =  96      7   300  16/8/16/32   8.9e-08  5.0e-07  4.2e-07 / 4.1e-07 / 4.4e-07 (9.9e-08)  5.7e-07  6.1e-07
   64, 32 x 4 = 128     31   300  16/8/16/32   8.3e-08  5.0e-07  7.4e-07 / 7.4e-07 / 7.4e-07 (1.1e-07)  5.2e-07  5.3e-07
   64, 32 x 4 = 128      7   300  16/8/16/32   8.3e-08  5.7e-07  4.8e-07 / 4.8e-07 / 4.8e-07 (9.8e-08)  6.2e-07  5.9e-07
  128, 16 x 2 =  32     31   300  8/8/16/32    9.7e-08  6.0e-07  5.1e-07 / 5.2e-07 / 5.2e-07 (3.8e-07)  5.3e-07  6.1e-07
  128, 16 x 2 =  32      7   300  8/8/16/32    8.2e-08  5.5e-07  6.1e-07 / 6.4e-07 / 6.2e-07 (4.1e-07)  5.8e-07  5.8e-07
  128, 32 x 1 =  32     31   300  8/8/16/32    1.0e-07  6.0e-07  5.3e-07 / 5.3e-07 / 5.4e-07 (3.2e-07)  6.4e-07  6.2e-07
  128, 32 x 1 =  32      7   300  8/8/16/32    8.5e-08  4.2e-07  5.1e-07 / 5.3e-07 / 5.1e-07 (3.9e-07)  4.5e-07  4.7e-07
  128, 16 x 3 =  48     31   300  16/8/16/32   9.2e-08  6.6e-07  8.4e-07 / 9.2e-07 / 9.3e-07 (7.4e-07)  7.1e-07  7.4e-07
  128, 16 x 3 =  48      7   300  16/8/16/32   9.3e-08  5.1e-07  4.9e-07 / 4.8e-07 / 4.8e-07 (4.1e-07)  5.2e-07  5.2e-07
  128, 32 x 2 =  64     31   300  16/16/16/32  9.1e-08  7.3e-07  9.6e-07 / 9.7e-07 / 9.6e-07 (1.1e-07)  7.8e-07  7.6e-07
  128, 32 x 2 =  64      7   300  16/16/16/32  8.1e-08  4.0e-07  7.8e-07 / 7.8e-07 / 7.7e-07 (1.2e-07)  4.6e-07  4.5e-07
  128, 16 x 4 =  64     31   300  16/16/16/32  8.2e-08  7.0e-07  9.5e-07 / 1.0e-06 / 9.8e-07 (1.9e-07)  7.7e-07  8.0e-07
  128, 16 x 4 =  64      7   300  16/16/16/32  8.1e-08  4.2e-07  4.2e-07 / 4.1e-07 / 4.0e-07 (1.4e-07)  4.3e-07  4.3e-07
  128, 32 x 3 =  96     31   300  16/16/16/32  8.7e-08  4.9e-07  8.4e-07 / 8.4e-07 / 8.3e-07 (1.2e-07)  4.9e-07  4.9e-07
  128, 32 x 3 =  96      7   300  16/16/16/32  8.4e-08  5.4e-07  4.9e-07 / 5.0e-07 / 5.0e-07 (9.8e-08)  6.5e-07  6.4e-07
  128, 32 x 4 = 128     31   300  16/16/16/32  9.1e-08  6.9e-07  5.8e-07 / 5.9e-07 / 5.9e-07 (7.2e-08)  7.0e-07  7.0e-07
  128, 32 x 4 = 128      7   300  16/16/16/32  8.2e-08  7.2e-07  5.4e-07 / 5.4e-07 / 5.3e-07 (8.1e-08)  7.9e-07  7.9e-07
   64, 32 x 4 = 128     31    31  16/8/16/32   7.6e-08  6.2e-06  7.3e-07 / 7.3e-07 / 7.3e-07 (2.7e-08)  6.2e-06  6.2e-06
   64, 32 x 4 = 128     31  1531  16/8/16/32   9.8e-08  3.7e-06  9.8e-07 / 9.5e-07 / 9.9e-07 (2.0e-07)  4.1e-06  3.5e-06
   64, 32 x 4 = 128      7    31  16/8/16/32   7.8e-08  4.6e-07  4.1e-07 / 4.1e-07 / 4.1e-07 (2.1e-08)  4.7e-07  5.0e-07
   64, 32 x 4 = 128      7  1531  16/8/16/32   9.8e-08  1.1e-06  1.1e-06 / 1.1e-06 / 1.1e-06 (2.0e-07)  1.1e-06  1.2e-06
  128, 32 x 4 = 128     31    31  16/16/16/32  9.5e-08  6.2e-07  5.3e-07 / 5.3e-07 / 5.3e-07 (2.2e-08)  6.1e-07  6.2e-07
  128, 32 x 4 = 128     31  1531  16/16/16/32  9.4e-08  1.7e-06  1.5e-06 / 1.6e-06 / 1.6e-06 (3.4e-07)  1.8e-06  1.8e-06
  128, 32 x 4 = 128      7    31  16/16/16/32  6.5e-08  4.2e-07  4.0e-07 / 4.0e-07 / 4.0e-07 (1.4e-08)  4.2e-07  4.2e-07
  128, 32 x 4 = 128      7  1531  16/16/16/32  9.4e-08  1.1e-06  1.2e-06 / 1.2e-06 / 1.2e-06 (2.3e-07)  1.1e-06  1.1e-06
  all 32 masks at  64, 32 x 4 (form 16): forward 8.5e-08, leg 1 7.9e-07, leg 2 2.3e-06 (2.0e-07)
  all 32 masks at 128, 16 x 2 (form  8): forward 8.3e-08, leg 1 1.5e-06, leg 2 1.0e-06 (4.1e-07)
  128, 32 x 4, time resolution 150, mask 31: forward 7.7e-08, leg 2 1.7e-06 / 1.7e-06 / 1.7e-06 (1.0e-07)
  leg 2 behind the forced weight-stationary forward (d1_form 8), worst of all rows above: 2.2e-06
The forms agree with plan_fwd's rule (expected_form below) in every row.
"""
import contextlib
import ctypes
import importlib
import json

import pytest
import torch

from conftest import set_knob
from scenes import rel_l2
from test_gpu_deform import _fdgs, _parity, _render_end_to_end_vs_oracle

pytestmark = pytest.mark.gpu
synthetic = importlib.import_module("4dgaussians_amd.synthetic")

CFG = "dynerf_default"                      # the named config the overrides start from (every field that matters is overridden)
RES = [16, 16, 16, 10]
HEAD_NAMES = ("pos_deform", "scales_deform", "rotations_deform", "opacity_deform", "shs_deform")
HEAD_FLAGS = ("no_dx", "no_ds", "no_dr", "no_do", "no_dshs")
GRIDS = [(16, [1, 2]), (32, [1]), (16, [1, 2, 4]), (32, [1, 2]), (16, [1, 2, 4, 8]), (32, [1, 2, 4]), (32, [1, 2, 4, 8])]
LEGS = ("default", "frame", "recompute", "form8", "form16", "form32")


def _overrides(W, multires, mask):
    ov = dict(net_width=W, multires=list(multires))
    ov.update({flag: not (mask >> h) & 1 for h, flag in enumerate(HEAD_FLAGS)})
    return ov


def _kw(case):
    W, C, multires, mask, n = case[:5]
    return dict(overrides=_overrides(W, multires, mask), kplanes=dict(output_coordinate_dim=C, resolution=list(case[5]) if len(case) > 5 else RES),
                candidates=4 * n + 64)


def _case_id(case):
    W, C, multires, mask, n = case[:5]
    return f"w{W}-c{C}-l{len(multires)}-m{mask}-n{n}" + ("-t150" if len(case) > 5 else "")


def expected_form(knob, W, C, L):
    """The forward form plan_fwd (csrc/deform.hip) chooses for d1_form = knob: has_fwd_ws is every C * L at net_width 64 and C * L <= 48 at
    net_width 128; by shape (knob 0) the weight-stationary form only at net_width 128 with up to two levels."""
    F = C * L
    if knob in (16, 32):
        return knob
    if knob == 8:
        return 8 if W == 64 or F <= 48 else 16
    return 8 if W == 128 and L <= 2 and F <= 48 else 16


@contextlib.contextmanager
def _timing_rows():
    """{kernel row: launches} of the library's own timing report over the block (the rows of earlier calls dropped first)."""
    lib = _fdgs()._lib
    L = lib.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    lib.check(L.fdgs_timing_report(buf, len(buf), 1))
    rows = {}
    L.fdgs_timing_enable(1)
    try:
        yield rows
        lib.check(L.fdgs_timing_report(buf, len(buf), 1))
        rows.update({l.split()[0]: int(l.split()[1]) for l in buf.value.decode().strip().splitlines()})
    finally:
        L.fdgs_timing_enable(0)


def _form_of(rows):
    """A deform_gather row: the weight-stationary form 8; a pack_weights row: form 16; neither: form 32 (fdgs_deform_fwd)."""
    assert rows.get("deform_fwd") == 1, rows
    return 8 if "deform_gather" in rows else 16 if "pack_weights" in rows else 32


# the CPU half (network, safe rows, oracle outputs and gradients) of the case that is running: built once per (case, time form), read-only
_current = {"case": None, "sides": {}}


def _shared(case, kind):
    if _current["case"] != case:
        _current["case"], _current["sides"] = case, {}
    return _current["sides"].setdefault(kind, {})


def _report(case, leg, **values):
    print("SHAPES-REPORT " + json.dumps(dict(case=_case_id(case), leg=leg, **values)))


def _worst(rep):
    return max(rep.values()) if rep else 0.0


def _reassociation_bound(numel):
    """test_dead_tile_skipping_is_exact's bounds for two HIP runs that add the same products in another order."""
    return 2e-5 if numel <= 64 else 1e-5 if numel <= 48 * 128 else 2e-6


def _frame_leg(case):
    """Leg 2: one frame time, rows declared ordered -> row lists and the matrix-core plane-gradient splat; as planned, with the 32-row
    backward-data kernel (d2_form = 32), with the per-corner plane-gradient kernel (d4_mfma = 0), and behind the weight-stationary forward
    where it has an instance (d1_form = 8: the weight-stationary backward-data kernel of net_width 128, C * L <= 48 then reads ITS saved
    activations).  Each against the oracle; the first two against each other."""
    n, kw, sh = case[4], _kw(case), _shared(case, "frame")
    tuning = _fdgs()._lib.tuning
    runs, worst = {}, {}
    for name, knobs in (("planned", {}), ("d2_form_32", dict(d2_form=32)), ("d4_atomics", dict(d4_mfma=0)),
                        ("d1_form_8", dict(d1_form=8))):
        runs[name] = {}
        with tuning(**knobs):
            worst[name] = _worst(_parity(CFG, n, True, scalar_time=0.37, ordered=True, shared=sh, details=runs[name], **kw))
    between = {}
    for k, a in runs["planned"]["grads"].items():
        b = runs["d2_form_32"]["grads"][k]
        assert (a is None) == (b is None), k
        if a is not None and float(b.abs().max()) > 0.0:
            between[k] = rel_l2(a.numpy(), b.numpy())
            assert between[k] < _reassociation_bound(a.numel()), (k, between[k])
    _report(case, "frame", fwd=_worst(runs["planned"]["fwd"]), grad=worst, planned_vs_d2_form_32=_worst(between))
    return runs["planned"]


def _leg(case, leg, monkeypatch):
    W, C, multires, mask, n = case[:5]
    if leg == "frame":
        return _frame_leg(case)
    knob = {"form8": 8, "form16": 16, "form32": 32}.get(leg, 0)
    if knob:
        set_knob("d1_form", knob)
    if leg == "recompute":
        monkeypatch.setattr(_fdgs().deformation, "SAVE_ACTIVATIONS", False)
    det = {}
    with _timing_rows() as rows:
        rep = _parity(CFG, n, True, shared=_shared(case, "rows"), details=det, **_kw(case))
    form = _form_of(rows)
    _report(case, leg, form=form, fwd=_worst(det["fwd"]), grad=_worst(rep))
    assert form == expected_form(knob, W, C, len(multires)), (form, rows)
    return det


# ---- every compiled shape --------------------------------------------------------------------------------------------------------------
SHAPE_CASES = [(W, C, tuple(mr), mask, 300) for W in (64, 128) for C, mr in GRIDS for mask in (31, 7)]
SHAPE_CASES += [(W, 32, (1, 2, 4, 8), mask, n) for W in (64, 128) for mask in (31, 7) for n in (31, 1531)]


@pytest.mark.parametrize("case,leg", [pytest.param(c, l, id=f"{_case_id(c)}-{l}") for c in SHAPE_CASES for l in LEGS])
def test_every_compiled_shape_against_the_oracle(case, leg, monkeypatch):
    """net_width {64, 128} x (C, levels) of GRIDS x head masks {31, 7}: forward and backward of every leg (module docstring) against the
    oracle, and the forward form that ran against plan_fwd's rule.  1531 rows run on 13 workgroups: the persistent loops of forms 8 / 16 / 32
    then end on leftover tiles."""
    if case[4] == 1531:
        set_knob("d1_wgs", 13)
    _leg(case, leg, monkeypatch)


def test_one_frame_time_with_large_time_planes():
    """net_width 128, C 32, four levels, time resolution 150 and no d4_rows_kb cap: the private time rows of the splat are 3 * C * res floats
    per level (one row per spatial texel of each time plane: the time resolution does not enter), 92 160 bytes for the four levels here,
    inside the 106 624 bytes the splat's fixed LDS leaves of 160 KB at C 32 (bwd_plane_grads, csrc/deform.hip): every level is privatised."""
    _frame_leg((128, 32, (1, 2, 4, 8), 31, 300, (16, 16, 16, 150)))


# ---- every head set --------------------------------------------------------------------------------------------------------------------
MASK_CASES = [(W, C, mr, mask, 300) for W, C, mr in ((64, 32, (1, 2, 4, 8)), (128, 16, (1, 2))) for mask in range(32)]


@pytest.mark.parametrize("case,leg", [pytest.param(c, l, id=f"{_case_id(c)}-{l}") for c in MASK_CASES for l in ("default", "frame")])
def test_every_head_set_against_the_oracle(case, leg, monkeypatch):
    """All 32 combinations of no_dx .. no_dshs at the reference's default shape and at (128, C 16, two levels): every mask but 31 and 7 takes
    the generic forward and the 32-row backward-data kernel with the active heads packed into slots.  Beside the parity of the leg: a
    disabled head's output is its input bit for bit (activate=False), and its parameters receive no gradient."""
    mask = case[3]
    det = _leg(case, leg, monkeypatch)
    for h, name in enumerate(HEAD_NAMES):
        for k, g in det["grads"].items():
            if f".{name}." in k and not (mask >> h) & 1:
                assert g is None or float(g.abs().max()) == 0.0, k
            elif f".{name}." in k:
                assert g is not None and float(g.abs().max()) > 0.0, k
    fd, dev = _fdgs(), torch.device("cuda:0")
    gi = [x.to(dev) for x in det["ins"]]
    time = gi[5] if leg == "default" else 0.37
    with torch.no_grad():
        raw = fd.deformation.deform(det["net"], *gi[:4], shs=gi[4], time=time, activate=False, ordered=leg == "frame")
    for h in range(5):
        assert torch.equal(raw[h], gi[h]) == (not (mask >> h) & 1), (h, mask)


@pytest.mark.parametrize("case", [pytest.param(c, id=_case_id(c)) for c in MASK_CASES if c[3] == 0])
@pytest.mark.parametrize("time", ["rows", "frame"])
def test_no_head_is_the_identity(case, time):
    """Mask 0: outputs are the inputs and the input gradients are the upstream gradients, bit for bit; no plane or MLP tensor gets a
    gradient."""
    fd, dev = _fdgs(), torch.device("cuda:0")
    det = {}
    _parity(CFG, case[4], False, scalar_time=None if time == "rows" else 0.37, ordered=time == "frame", details=det, **_kw(case))
    gi = [x.to(dev).requires_grad_(i < 5) for i, x in enumerate(det["ins"])]
    out = fd.deformation.deform(det["net"], *gi[:4], shs=gi[4], time=gi[5] if time == "rows" else 0.37, activate=False, ordered=time == "frame")
    ws = [torch.randn(o.shape, generator=torch.Generator().manual_seed(6)).to(dev) for o in out]
    params = [p for p in det["net"].parameters() if p.requires_grad]
    grads = torch.autograd.grad(sum((o * w).sum() for o, w in zip(out, ws)), gi[:5] + params, allow_unused=True)
    for o, x, g, w in zip(out, gi, grads, ws):
        assert torch.equal(o.detach(), x.detach()) and torch.equal(g, w.reshape(g.shape))
    for g in grads[5:]:
        assert g is None or float(g.abs().max()) == 0.0


# ---- render() end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,overrides", [
    pytest.param("dnerf_bouncingballs", dict(net_width=64, defor_depth=1, multires=[1, 2, 4, 8]), id="reference-defaults-mask7"),
    pytest.param("dynerf_default", dict(net_width=128, multires=[1, 2, 4], no_ds=True, no_dr=True), id="w128-f96-heads-x-o-shs")])
def test_render_end_to_end_at_other_shapes_and_head_sets(cfg, overrides):
    """The fine stage of render() -- implicit Hilbert order, fused deformation epilogue of the rasterizer backward, whose packed gradient
    rows depend on the head set -- at the reference's default shape (net_width 64, C 32, four levels, position / scale / rotation) and at
    net_width 128, C * L = 96 with the position, opacity and SH heads.  Bounds of _render_end_to_end_vs_oracle."""
    _render_end_to_end_vs_oracle(cfg, "fine", overrides=overrides, kplanes=dict(output_coordinate_dim=32, resolution=RES))


# ---- a shape without a compiled instance -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [64, 128])
def test_unsupported_shape_fails_cleanly(W):
    """C 16 with one level (C * L = 16) passes validate_deform and has no instance in dispatch_wf: forward and backward return an error that
    names the combination, and the next supported call on the same stream is unharmed."""
    fd, dev = _fdgs(), torch.device("cuda:0")
    D, lib = fd.deformation, fd._lib
    n = 300
    torch.manual_seed(3)
    args = synthetic.deform_args(CFG, **_overrides(W, [1], 31))
    args.kplanes_config.update(output_coordinate_dim=16, resolution=RES)
    net = fd.deform_network(args).to(dev)
    g = synthetic.make_gaussians(n, seed=3)
    ins = [x.to(dev) for x in (g["xyz"], g["scaling"], g["rotation"], g["opacity"], torch.cat([g["features_dc"], g["features_rest"]], 1))]
    with pytest.raises(lib.FdgsError, match=r"unsupported \(net_width, C\*L\) combination"):
        D.deform(net, *ins[:4], shs=ins[4], time=0.37, activate=False)
    # the backward as _DeformFunction.backward runs it, on a forward state put together by hand (no forward got that far); nothing saved
    planes, mlp = D._collect(net)
    cfg = D._forward_cfg(net.deformation_net, ins[0], False, ordered=False)
    cfg["save"] = False
    st = D._FwdState()
    st.cfg, st.keep, st.saved_act, st.o_norm = cfg, [], None, None
    st.p = D._fill_params(cfg, 0.37, *ins[:4], ins[4], None, None, D._aabb_to_host(net.deformation_net.grid.aabb),
                          [D._cl(p.detach()) for p in planes], [m.detach() for m in mlp], st.keep)
    st.shapes = dict(scales=ins[1].shape, rot=ins[2].shape, op=ins[3].shape, sh_a=ins[4].shape, sh_b=None)
    st.plane_shapes = [tuple(p.shape) for p in planes]
    b = D.backward_prepare(st, None, None, None)
    ups = [torch.randn(x.shape, generator=torch.Generator().manual_seed(7)).to(dev) for x in ins]
    b.g.g_xyz, b.g.g_scales, b.g.g_rotations, b.g.g_opacity, b.g.g_shs = map(lib.ptr, ups)
    with pytest.raises(lib.FdgsError, match=r"unsupported \(net_width, C\*L\) combination"):
        D.backward_run(st, b)
    torch.cuda.synchronize()
    _parity(CFG, n, True, **_kw((W, 16, (1, 2), 31, n)))
