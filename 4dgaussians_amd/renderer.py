"""Drop-in for `gaussian_renderer.render` of the reference (gaussian_renderer/__init__.py:18-138).

Same signature, same result dict {"render","viewspace_points","visibility_filter","radii","depth"} (and, opt-in through
`pipe.render_alpha = True`, "alpha": the accumulated opacity [1,H,W], differentiable; `pipe.antialiasing = True` compensates every opacity
for the 0.3 px dilation of its footprint, upstream's `antialiasing`; `pipe.absgrad = True` leaves the absolute screen-space gradients of every
backward on the frame's "viewspace_points" as `.absgrad` [P,3], the densification statistic of AbsGS); honours
pipe.convert_SHs_python / pipe.compute_cov3D_python / pipe.debug and cam_type == "PanopticSports" exactly where the
reference does.  When `pc._deformation` is this package's `deform_network`, the fine stage runs as two fused HIP
stages: deform(+activations, + the cat of features_dc/features_rest) -> rasterize; no `time.repeat(N,1)` tensor, no
positional-embedding scratch.  With a foreign deformation module (e.g. the reference's own) the module is called as
the reference calls it and only the rasterizer is replaced.
"""
import math
import os

import torch

from . import _lib
from . import deformation as _deformation
from . import rasterizer as _rasterizer
from .rasterizer import FrameOptions, GaussianRasterizationSettings, GaussianRasterizer

# Fused fine stage: deformation and rasterizer behind ONE autograd node, so that the rasterizer backward's per-Gaussian chain rule
# writes straight into the deformation backward's buffers (fdgs_raster_deform_epilogue) instead of handing five gradient tensors
# through autograd to a separate packing kernel.  FDGS_FUSED_BACKWARD=0 keeps the two-node form (A/B, and what the tests compare with).
FUSED_BACKWARD = os.environ.get("FDGS_FUSED_BACKWARD", "1") != "0"
EPILOGUE_ASSIGN = True     # False: the epilogue accumulates (+=) into a zero-filled arena (the C-ABI's other mode; tests compare both)
# fdgs_raster_deform_epilogue::tile_flags of the fused backward.  None = 2 (dead tiles' rows unwritten, always skipped) unless the library's
# tuning knob skip_dead = 0 asks for every tile to be walked (then 1: flags written, every row written).  0 / 1 / 2 force a mode (tests).
# The deformation backward is told which mode produced its rows (packed_rows_ready = tile_flags + 1), never the environment alone.
EPILOGUE_TILE_FLAGS = None


# The spatial order kept inside the library: a model whose rows are NOT spatial neighbours (the reference's own densify / prune appends at
# the tail) is read through a cached Hilbert permutation of its positions (deformation.implicit_permutation); radii, visibility and the
# per-Gaussian gradients come back in the model's own order.  FDGS_IMPLICIT_ORDER=0 switches it off (the A/B figure `random_order` of bench.py).
IMPLICIT_ORDER = os.environ.get("FDGS_IMPLICIT_ORDER", "1") != "0"
IMPLICIT_ORDER_MIN_N = 8192


def _implicit_perm(pc, cfg, dn):
    if IMPLICIT_ORDER and not cfg["ordered"] and pc._xyz.shape[0] >= IMPLICIT_ORDER_MIN_N:
        # fdgs_permute_rows moves rows of 4-byte elements: a model that keeps any of these in another dtype (half-precision SH, say) takes
        # the unpermuted path, which accepts them
        if all(t.dtype == torch.float32 for t in (pc._xyz, pc._scaling, pc._rotation, pc._opacity, pc._features_dc, pc._features_rest)):
            return _deformation.implicit_permutation(pc._xyz, dn.grid.aabb)
    return None


def _fine_stage(pc, lead=()):
    """What the fused fine stage of one frame runs on -> (cfg, perm, per-Gaussian inputs, network inputs).  The inputs are `lead` (the
    gradient sinks of the screen-space means) and the model's six arrays; where the set is read through the implicit Hilbert permutation
    they are permuted here (gradients come back through the inverse; detached when no graph is recorded) and cfg["ordered"] is set.
    render(), render_views() and the baked playback all deform through this, which is what keeps a baked frame render()'s own."""
    net = pc._deformation
    planes, mlp = _deformation._collect(net)
    dn = net.deformation_net
    cfg = _deformation._forward_cfg(dn, pc._xyz, True)
    ins = (*lead, pc.get_xyz, pc._scaling, pc._rotation, pc._opacity, pc._features_dc, pc._features_rest)
    perm = _implicit_perm(pc, cfg, dn)
    if perm is not None:
        cfg["ordered"] = True
        ins = _deformation.PermuteRows.apply(perm, *ins) if cfg["grad"] else tuple(_deformation.permute_rows(perm, [t.detach() for t in ins]))
    return cfg, perm, ins, (dn.grid.aabb, *planes, *mlp)


def _time_value(t):
    """The frame time as the number the kernels take by value (a tensor: one host read)."""
    return float(t.detach()) if isinstance(t, torch.Tensor) else float(t)


def _frame_settings(camera, cam_type, bg_color, scaling_modifier, sh_degree, device, pipe):
    """(GaussianRasterizationSettings, frame time) of one camera, as gaussian_renderer/__init__.py:31-58 builds them: a "PanopticSports"
    camera is a dict that brings its settings along."""
    if cam_type == "PanopticSports":
        return camera["camera"], _time_value(camera["time"])
    return GaussianRasterizationSettings(
        image_height=int(camera.image_height), image_width=int(camera.image_width), tanfovx=math.tan(camera.FoVx * 0.5),
        tanfovy=math.tan(camera.FoVy * 0.5), bg=bg_color, scale_modifier=scaling_modifier,
        viewmatrix=_dev(camera.world_view_transform, device), projmatrix=_dev(camera.full_proj_transform, device),
        sh_degree=sh_degree, campos=_dev(camera.camera_center, device), prefiltered=False, debug=pipe.debug), _time_value(camera.time)


def _tile_flags():
    if EPILOGUE_TILE_FLAGS is not None:
        return int(EPILOGUE_TILE_FLAGS)
    return 2 if _lib.tuning_get("skip_dead") != 0 else 1


def _fill_epilogue(st, b, assign):
    """The fdgs_raster_deform_epilogue of one view's rasterizer backward: its per-Gaussian chain rule writes straight into the deformation
    backward's buffers `b` (assign: the identity paths are assigned, not accumulated into)."""
    epi = _lib.RasterDeformEpilogue()
    epi.activate, epi.Npad = 1, (st.p.N + 127) // 128 * 128
    epi.rot_norm, epi.G = _lib.ptr(st.o_norm), _lib.ptr(b.scratch)
    epi.d_xyz, epi.d_scales, epi.d_rotations, epi.d_opacity = b.g.d_xyz, b.g.d_scales, b.g.d_rotations, b.g.d_opacity
    epi.d_shs_dc, epi.d_shs_rest = b.g.d_shs_dc, b.g.d_shs_rest
    epi.shs_dc_stride, epi.shs_rest_stride = st.p.shs_dc_stride, st.p.shs_rest_stride
    epi.assign = 1 if assign else 0
    epi.tile_flags = _tile_flags()      # per-tile non-zero flags behind the packed rows; 2: rows of dead tiles stay unwritten
    if b.zero_range is not None:        # the accumulate-into part of the gradient arena is cleared by the epilogue kernel on the way
        epi.zero_fill, epi.zero_floats = b.zero_range
    return epi


def _fused_backward(states, saved, grad_colors, grad_depths, grad_alphas, camera=False, time=False, zero_by_epilogue=False):
    """The backward of the fused fine stage for the views of one autograd node: states = [(deformation state, raster state)], saved = their
    (o_sc, o_rot, o_op) in a row, grad_colors / grad_depths / grad_alphas = the per-view image gradients (or None; alpha: frames rendered
    with it), `zero_by_epilogue` goes to backward_prepare.
    Last view first (its saved activations, lists and records are the ones still partly resident in the 256 MB Infinity Cache), per view: the
    rasterizer backward, whose epilogue writes into the ONE gradient arena (the first processed view assigns the identity paths, later ones
    accumulate), then that view's deformation backward -- same output pointers and scratch (stream-ordered reuse), its own saved activations.
    `camera`: per view also the 48 floats of fdgs_camera_grad, run behind that view's fdgs_raster_bwd on its accumulator.  `time`: per view
    also the [1] tensor of fdgs_deform_time_grad, run behind that view's fdgs_deform_bwd.
    Views rendered with absgrad also get their [P,3] absolute screen-space gradients (fdgs_raster_bwd_abs: the same launches).
    Returns ([d means2D per view], the arena's views in _DeformFunction's input order, [camera rows per view], [time rows per view],
    [absolute rows per view]); the last three hold None where not asked for."""
    L, stream = _lib.lib(), _lib.stream_ptr()
    st0 = states[0][0]
    b = _deformation.backward_prepare(st0, saved[0], saved[1], saved[2], identity_assigned=EPILOGUE_ASSIGN, zero_by_epilogue=zero_by_epilogue)
    dev = b.d_xyz.device
    g_means2D, cam_rows, time_rows, keep = [None] * len(states), [None] * len(states), [None] * len(states), []
    abs_rows = [None] * len(states)
    for k_, v in enumerate(reversed(range(len(states)))):
        st, rstate = states[v]
        p = rstate.params
        gc = _lib.f32(grad_colors[v]) if grad_colors is not None else torch.zeros(3, p.H, p.W, device=dev)
        gd = _lib.f32(grad_depths[v]) if grad_depths is not None else None
        ga = _lib.f32(grad_alphas[v]) if grad_alphas is not None else None
        gm = g_means2D[v] = torch.empty(p.P, 3, device=dev)
        epi = _fill_epilogue(st, b, EPILOGUE_ASSIGN and k_ == 0)
        g, acc = _rasterizer.fill_raster_grads(rstate, gc, gd, gm, epi)      # (acc: zero-filled by the blending forward of this frame, no fill launch here)
        if rstate.absgrad:
            abs_rows[v] = torch.empty(p.P, 3, device=dev)
        _rasterizer.raster_bwd_call(L, rstate, g, ga, abs_rows[v])
        if camera:
            cam_rows[v] = _rasterizer.camera_gradients(rstate, acc)
        b.g.out_scales, b.g.out_rotations, b.g.out_opacity = _lib.ptr(saved[3 * v]), _lib.ptr(saved[3 * v + 1]), _lib.ptr(saved[3 * v + 2])
        b.g.rot_norm, b.g.saved = _lib.ptr(st.o_norm), _lib.ptr(st.saved_act)
        b.g.packed_rows_ready = epi.tile_flags + 1
        _lib.check(L.fdgs_deform_bwd(stream, st.p, b.g))
        _deformation.note_live_tiles(st, b)
        if time:
            time_rows[v] = _deformation.time_gradient(st, b)
        keep.append((gc, gd, ga, acc, epi))      # (what the queued launches read lives until the last of them is queued)
    return g_means2D, _deformation.gradient_tuple(st0, b), cam_rows, time_rows, abs_rows


def _view_forward(cfg, opts, t_scalar, raster_settings, tensors, want, out=None):
    """One view of the fused fine stage: the deformation at `t_scalar`, then the rasterizer on its outputs -> (deformation state,
    rasterize_forward's result).  `tensors` = (xyz, scales, rotations, opacity, sh_a, sh_b, aabb, planes..., mlp...); `want`: a backward will
    follow; `out`: rasterize_forward's.  The one place render(), its nodes and render_views() go through, with the frame's FrameOptions."""
    st = _deformation.forward_impl(cfg, t_scalar, *tensors[:6], None, tensors[6], tensors[7:], want)
    res = _rasterizer.rasterize_forward(raster_settings, st.o_xyz, st.o_sh, None, st.o_op, st.o_sc, st.o_rot, None, out=out,
                                        expect_backward=bool(cfg.get("grad")) and want, **opts.keywords())
    st.o_xyz = st.o_sh = None
    return st, res


# ---- the autograd nodes of the fused fine stage ----------------------------------------------------------------------------------------------
# One forward and one backward body (_node_forward, _node_backward); each single-view class is the signature its frames record, around
# them.  Separate classes, so that a frame whose camera or time does not ask for a gradient records the node, with the inputs, it always
# recorded -- autograd.Function.apply has a per-input cost (render(): the no-grad branch) -- and makes the C calls it always made.

def _absgrad_sinks(cfg, opts):
    """Where the backward of an absgrad frame leaves its rows: (the views' gradient sinks as the caller holds them, the permutation the set
    was read through or None), put into the frame's own `cfg` by render() / render_views() -- the node's inputs are the PERMUTED sinks
    where the implicit order is on, and the rows have to reach the caller's leaves in the model's row order."""
    return cfg.get("absgrad_sinks") if opts.absgrad else None


def _node_forward(ctx, cfg, opts, t_scalar, raster_settings, tensors, want):
    st, (color, radii, depth, *alpha, rstate) = _view_forward(cfg, opts, t_scalar, raster_settings, tensors, want)
    ctx.states = [(st, rstate)]
    ctx.absgrad_sinks = _absgrad_sinks(cfg, opts)
    ctx.save_for_backward(st.o_sc, st.o_rot, st.o_op)       # (see deformation._node_forward: no reference cycle through ctx)
    st.o_sc = st.o_rot = st.o_op = None
    vis = rstate.visibility                                 # radii > 0, written by the projection kernel itself
    ctx.mark_non_differentiable(radii, vis)
    ctx.set_materialize_grads(False)
    return (color, radii, depth, vis, *alpha)               # (alpha: where the frame asked)


def _node_backward(ctx, image_grads, sink_at, cam_at=None, time_at=None, zero_by_epilogue=False):
    """One gradient per input of the node.  `image_grads` = the (colour, depth, alpha) gradients, each indexed by view or None.  Where the
    inputs sit: `sink_at` the gradient sinks of the screen-space means, one per view, with the model's six arrays, the aabb and the network
    behind them to the end; `cam_at` viewmatrix, projmatrix and campos (ctx.cam), `time_at` the time (ctx.time_like), in the nodes that have
    them.  Everything in front is no tensor."""
    out = [None] * len(ctx.needs_input_grad)
    if all(g is None for g in image_grads):                 # no image reached the loss
        return tuple(out)
    camera = cam_at is not None and any(ctx.needs_input_grad[cam_at:cam_at + 3])
    g_means2D, grads, cam_rows, time_rows, abs_rows = _fused_backward(ctx.states, ctx.saved_tensors, *image_grads, camera=camera,
                                                                      time=time_at is not None, zero_by_epilogue=zero_by_epilogue)
    if ctx.absgrad_sinks is not None:       # (back through the scatter the signed rows take in PermuteRows.backward: the model's row order)
        sinks, perm = ctx.absgrad_sinks
        if perm is not None:
            abs_rows = _deformation.permute_rows(perm, abs_rows, scatter=True)
        for sink, rows in zip(sinks, abs_rows):
            _rasterizer.leave_absgrad(sink, rows)
    model_at = sink_at + len(g_means2D)
    out[sink_at:model_at] = g_means2D
    out[model_at:] = grads[:6] + grads[7:]                  # (grads[6]: the deformation's time tensor, no input of these nodes)
    if camera:
        out[cam_at:cam_at + 3] = _rasterizer.split_camera_gradients(cam_rows[0], *ctx.cam)
    if time_at is not None:
        out[time_at] = _deformation.time_gradient_like(time_rows[0], ctx.time_like)
    return tuple(out)


def _one_view(*image_grads):
    return [None if g is None else (g,) for g in image_grads]


class _FusedRenderFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, opts, t_scalar, raster_settings, means2D, *tensors):
        return _node_forward(ctx, cfg, opts, t_scalar, raster_settings, tensors, any(ctx.needs_input_grad))

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth, grad_vis=None, grad_alpha=None):
        # one view; the epilogue kernel also clears the accumulate-into part of the arena on the way
        return _node_backward(ctx, _one_view(grad_color, grad_depth, grad_alpha), sink_at=4, zero_by_epilogue=EPILOGUE_ASSIGN)


class _FusedRenderCameraFunction(torch.autograd.Function):
    """The node of a frame whose camera asks for a gradient (rasterizer.camera_wants_grad): viewmatrix, projmatrix and campos of the
    settings are inputs too and get the gradients of fdgs_camera_grad, run behind the same fdgs_raster_bwd."""

    @staticmethod
    def forward(ctx, cfg, opts, t_scalar, raster_settings, viewmatrix, projmatrix, campos, means2D, *tensors):
        ctx.cam = (viewmatrix, projmatrix, campos)
        return _node_forward(ctx, cfg, opts, t_scalar, raster_settings, tensors, True)

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth, grad_vis=None, grad_alpha=None):
        return _node_backward(ctx, _one_view(grad_color, grad_depth, grad_alpha), sink_at=7, cam_at=4, zero_by_epilogue=EPILOGUE_ASSIGN)


class _FusedRenderTimeFunction(torch.autograd.Function):
    """The node of a frame whose time asks for a gradient (a scalar tensor that requires grad: fdgs.camera.TimeDelta, tracking a time against
    a frozen model): the time is an input and gets the [1] result of fdgs_deform_time_grad, run behind the same fdgs_deform_bwd; viewmatrix,
    projmatrix and campos are inputs too and get fdgs_camera_grad's where one of them asks (joint pose and time).  `t_scalar` is the time's
    value, read on the host by the caller."""

    @staticmethod
    def forward(ctx, cfg, opts, t_scalar, raster_settings, time, viewmatrix, projmatrix, campos, means2D, *tensors):
        ctx.cam, ctx.time_like = (viewmatrix, projmatrix, campos), _deformation.time_like(time)
        return _node_forward(ctx, cfg, opts, t_scalar, raster_settings, tensors, True)

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth, grad_vis=None, grad_alpha=None):
        return _node_backward(ctx, _one_view(grad_color, grad_depth, grad_alpha), sink_at=8, cam_at=5, time_at=4, zero_by_epilogue=EPILOGUE_ASSIGN)


class _FusedRenderViewsFunction(torch.autograd.Function):
    """The `batch_size` views of one optimizer step (train.py:180-201) behind ONE autograd node: every view's backward accumulates into
    the SAME gradient arena (first view: the epilogue assigns the per-Gaussian identity paths, later views accumulate), so a step pays
    one arena allocation / zero fill and no per-parameter `grad += grad` kernels (the per-view graph costs 40 of them per extra view)."""

    @staticmethod
    def forward(ctx, cfg, opts, times, settings_list, nviews, *tensors):
        tensors = tensors[nviews:]          # (behind the views' gradient sinks: xyz, scales, rotations, opacity, sh_a, sh_b, aabb, network)
        want = any(ctx.needs_input_grad)
        dev, P = tensors[0].device, tensors[0].shape[0]
        H, W = int(settings_list[0].image_height), int(settings_list[0].image_width)
        colors = torch.empty(nviews, 3, H, W, device=dev)          # every view renders straight into its slice
        radii_all = torch.empty(nviews, P, dtype=torch.int32, device=dev)
        depths = torch.empty(nviews, 1, H, W, device=dev)
        outs = (colors, radii_all, depths) + ((torch.empty(nviews, 1, H, W, device=dev),) if opts.alpha else ())
        states = []
        for v in range(nviews):
            st, (*_, rstate) = _view_forward(cfg, opts, times[v], settings_list[v], tensors, want, out=tuple(o[v] for o in outs))
            states.append((st, rstate))
        ctx.states = states
        ctx.absgrad_sinks = _absgrad_sinks(cfg, opts)
        # the activated outputs each view's backward needs: through save_for_backward (no reference cycle through ctx)
        ctx.save_for_backward(*[t for st, _ in states for t in (st.o_sc, st.o_rot, st.o_op)])
        for st, _ in states:
            st.o_sc = st.o_rot = st.o_op = None
        ctx.mark_non_differentiable(radii_all)
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    def backward(ctx, grad_colors, grad_radii, grad_depths, grad_alphas=None):
        return _node_backward(ctx, (grad_colors, grad_depths, grad_alphas), sink_at=5)


def render_views(viewpoint_cameras, pc, pipe, bg_color, scaling_modifier=1.0, stage="fine", cam_type=None):
    """The views of one optimizer step rendered behind one autograd node: `[render(cam, ...) for cam in viewpoint_cameras]` of the
    reference's batch loop (train.py:180-198) with the same per-view result dicts, but one gradient arena for the whole step (see
    _FusedRenderViewsFunction).  Falls back to per-view render() wherever the fused fine stage does not apply.
    The views' times are taken as numbers: a time tensor that requires grad gets its gradient from render(), not from here."""
    cams = list(viewpoint_cameras)
    fusable = (FUSED_BACKWARD and "fine" in stage and isinstance(pc._deformation, _deformation.deform_network)
               and not pipe.compute_cov3D_python and not pipe.convert_SHs_python and len(cams) > 0)
    if not fusable:
        return [render(c, pc, pipe, bg_color, scaling_modifier, None, stage, cam_type) for c in cams]
    means3D = pc.get_xyz
    device = means3D.device
    settings, times = zip(*[_frame_settings(cam, cam_type, bg_color, scaling_modifier, pc.active_sh_degree, device, pipe) for cam in cams])
    if len({(s_.image_height, s_.image_width) for s_ in settings}) != 1:
        return [render(c, pc, pipe, bg_color, scaling_modifier, None, stage, cam_type) for c in cams]
    sinks = [_zero_leaf(means3D) for _ in cams]
    cfg, perm, ins, net_ins = _fine_stage(pc, sinks)       # (the set in Hilbert order for this step where perm is not None)
    opts = FrameOptions.of(pipe)
    if opts.absgrad:
        cfg["absgrad_sinks"] = (sinks, perm)
    colors, radii, depths, *alphas = _FusedRenderViewsFunction.apply(cfg, opts, times, settings, len(cams), *ins, *net_ins)
    if perm is not None:
        radii = torch.stack(_deformation.permute_rows(perm, [radii[v] for v in range(len(cams))], scatter=True))
    res = [{"render": colors[v], "viewspace_points": sinks[v], "visibility_filter": radii[v] > 0, "radii": radii[v], "depth": depths[v]}
           for v in range(len(cams))]
    for v, r in enumerate(res if alphas else ()):
        r["alpha"] = alphas[0][v]
    return res


_zero_pool = {}


def _zero_leaf(like):
    """A fresh LEAF of zeros shaped like `like` without a fill launch per frame: every frame's leaf is a detached alias of one cached,
    never-written zero buffer per (shape, dtype, device) -- the values are only ever read (the rasterizer ignores them, as the reference's
    does), the gradient arrives in the leaf's own `.grad`.  READ-ONLY by contract: `viewspace_points` of every frame shares this storage, so
    an in-place write through it (`.data`, an op under no_grad) would show up in every later frame's tensor (the reference's is a fresh
    `zeros_like` per frame; nothing in the reference writes to it, train.py:223-225 only reads `.grad`)."""
    key = (tuple(like.shape), like.dtype, like.device)
    z = _zero_pool.get(key)
    if z is None:
        if len(_zero_pool) > 8:
            _zero_pool.clear()
        # (a normal tensor whatever mode the first caller is in: under torch.inference_mode() it would be an inference tensor and the
        # requires_grad_ of a later training frame would raise)
        with torch.inference_mode(False), torch.no_grad():
            z = _zero_pool[key] = torch.zeros(like.shape, dtype=like.dtype, device=like.device)
    if torch.is_inference_mode_enabled():
        return z.detach()                       # (no autograd inside inference mode: nothing will ask for a gradient)
    return z.detach().requires_grad_(True)


def _dev(t, device):
    return t if t.device == device else t.to(device, non_blocking=True)


def _time_leaf(camera, cam_type):
    """The camera's time where it asks for a gradient -- a one-element tensor that requires grad while a graph is recorded -- else None."""
    t = camera["time"] if cam_type == "PanopticSports" else camera.time
    return t if _deformation.time_wants_grad(t) and t.numel() == 1 else None


def render(viewpoint_camera, pc, pipe, bg_color, scaling_modifier=1.0, override_color=None, stage="fine", cam_type=None):
    """`viewpoint_camera.time` is a number or -- opt-in -- a one-element tensor that requires grad (fdgs.camera.TimeDelta): the fine stage
    then also returns dL/dt into it (fdgs_deform_time_grad, reduced in HIP), the coarse stage, which does not read the time, a zero.  The
    kernels take the time by value: such a tensor is read on the host once per frame (one `.item()`, on this opt-in path only)."""
    means3D = pc.get_xyz
    device = means3D.device
    # gradient sink for the screen-space means (train.py:223-225 reads .grad of this tensor).  A LEAF of zeros: the reference's
    # `zeros_like(...) + 0` with retain_grad() costs an extra add kernel per frame plus a clone of the gradient in the retain hook;
    # a leaf's .grad is filled by AccumulateGrad directly (same values, same attribute, read the same way by the train loop)
    screenspace_points = _zero_leaf(means3D)
    raster_settings, frame_time = _frame_settings(viewpoint_camera, cam_type, bg_color, scaling_modifier, pc.active_sh_degree, device, pipe)
    # opt-in: "alpha" [1,H,W], the accumulated opacity, joins the result (differentiable); antialiasing; absgrad (viewspace_points.absgrad)
    opts = FrameOptions.of(pipe)
    time_leaf = _time_leaf(viewpoint_camera, cam_type)      # opt-in: the frame time as something to fit (None: every frame there was before)
    if ("fine" in stage and "coarse" not in stage and FUSED_BACKWARD and override_color is None and not pipe.compute_cov3D_python
            and not pipe.convert_SHs_python and isinstance(pc._deformation, _deformation.deform_network)):
        # deformation + rasterizer as one autograd node (see _FusedRenderFunction)
        cfg, perm, ins, net_ins = _fine_stage(pc, (screenspace_points,) if torch.is_grad_enabled() else ())
        if opts.absgrad:
            cfg["absgrad_sinks"] = ((screenspace_points,), perm)
        if cfg["grad"] and time_leaf is not None:
            rs = raster_settings
            rendered_image, radii, depth, vis, *alpha = _FusedRenderTimeFunction.apply(cfg, opts, frame_time, rs, time_leaf, rs.viewmatrix,
                                                                                       rs.projmatrix, rs.campos, *ins, *net_ins)
        elif cfg["grad"] and _rasterizer.camera_wants_grad(raster_settings):
            rs = raster_settings
            rendered_image, radii, depth, vis, *alpha = _FusedRenderCameraFunction.apply(cfg, opts, frame_time, rs, rs.viewmatrix, rs.projmatrix,
                                                                                         rs.campos, *ins, *net_ins)
        elif cfg["grad"]:
            rendered_image, radii, depth, vis, *alpha = _FusedRenderFunction.apply(cfg, opts, frame_time, raster_settings, *ins, *net_ins)
        else:
            # no graph will be recorded (render.py:57-70, evaluation): the two stages called directly -- autograd.Function.apply costs
            # 0.05 ms per frame for its 46 inputs even when it has nothing to record
            _, (rendered_image, radii, depth, *alpha, rstate) = _view_forward(cfg, opts, frame_time, raster_settings, (*ins, *net_ins), False)
            vis = rstate.visibility
        if perm is not None:       # (radii and visibility back in the model's own row order)
            radii, = _deformation.permute_rows(perm, [radii], scatter=True)
            vis = radii > 0
        res = {"render": rendered_image, "viewspace_points": screenspace_points, "visibility_filter": vis, "radii": radii, "depth": depth}
        if alpha:
            res["alpha"] = alpha[0]
        return res

    means2D = screenspace_points
    opacity = pc._opacity
    scales = rotations = cov3D_precomp = None
    if pipe.compute_cov3D_python:
        cov3D_precomp = pc.get_covariance(scaling_modifier)
    else:
        scales, rotations = pc._scaling, pc._rotation

    fused = isinstance(pc._deformation, _deformation.deform_network) and not pipe.compute_cov3D_python
    if "coarse" in stage:
        means3D_final, shs_final = means3D, pc.get_features
        scales_final = None if scales is None else pc.scaling_activation(scales)
        rotations_final = None if rotations is None else pc.rotation_activation(rotations)
        opacity_final = pc.opacity_activation(opacity)
    elif "fine" in stage:
        if fused:
            means3D_final, scales_final, rotations_final, opacity_final, shs_final = _deformation.deform(
                pc._deformation, means3D, scales, rotations, opacity, shs_dc=pc._features_dc, shs_rest=pc._features_rest,
                time=frame_time if time_leaf is None else time_leaf.reshape(()), activate=True)
        else:
            time = (torch.tensor(frame_time) if time_leaf is None else time_leaf.reshape(1, 1)).to(device).repeat(means3D.shape[0], 1)
            means3D_final, scales_final, rotations_final, opacity_final, shs_final = pc._deformation(
                means3D, scales, rotations, opacity, pc.get_features, time)
            scales_final = None if scales_final is None else pc.scaling_activation(scales_final)
            rotations_final = None if rotations_final is None else pc.rotation_activation(rotations_final)
            opacity_final = pc.opacity_activation(opacity_final)
    else:
        raise NotImplementedError

    colors_precomp = None
    if override_color is None:
        if pipe.convert_SHs_python:
            # python SH path of the reference (gaussian_renderer/__init__.py:106-111): basis polynomial of
            # utils/sh_utils.py:57-112 evaluated with torch ops, colours handed to the rasterizer precomputed
            from .sh import eval_sh
            feats = pc.get_features
            shs_view = feats.transpose(1, 2).view(-1, 3, (pc.max_sh_degree + 1) ** 2)
            dir_pp = pc.get_xyz - _dev(viewpoint_camera.camera_center, device).repeat(feats.shape[0], 1)
            dir_pp = dir_pp / dir_pp.norm(dim=1, keepdim=True)
            colors_precomp = torch.clamp_min(eval_sh(pc.active_sh_degree, shs_view, dir_pp) + 0.5, 0.0)
            shs_final = None
    else:
        colors_precomp = override_color
        shs_final = None

    rasterizer = GaussianRasterizer(raster_settings=raster_settings, render_alpha=opts.alpha)       # (an nn.Module: only built on the paths that call it)
    if opts.antialiasing:
        rasterizer.antialiasing = True
    if opts.absgrad:
        rasterizer.absgrad = True
    rendered_image, radii, depth, *alpha = rasterizer(
        means3D=means3D_final, means2D=means2D, shs=shs_final, colors_precomp=colors_precomp, opacities=opacity_final,
        scales=scales_final, rotations=rotations_final, cov3D_precomp=cov3D_precomp)
    if time_leaf is not None and "coarse" in stage:      # (the coarse stage does not read the time: its gradient is a zero, not a missing one)
        rendered_image = rendered_image + (time_leaf * 0).sum().to(device=rendered_image.device, dtype=rendered_image.dtype)
    res = {"render": rendered_image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0,
           "radii": radii, "depth": depth}
    if alpha:
        res["alpha"] = alpha[0]
    return res
