"""Baked playback: render a trained 4D model from deformed states that stay resident in device memory.

The deformed, activated state of the Gaussians depends on the frame time only, never on the camera.  `render.py`'s loop, a viewer or a
video orbit re-evaluate the HexPlane gather and the deformation MLP for every frame all the same; `bake` runs them ONCE per timestamp and
`Baked.render` is the rasterizer alone (stages 1-4 of include/fdgs.h) on the stored state:

    baked = fdgs.playback.bake(gaussians, times)                              # once: len(times) deformation forwards
    for cam in cameras:
        out = baked.render(cam, pipe, background, rgb8="trunc")               # render.py:57-70 -- out["render"], out["rgb8"]

    fdgs.playback.export_ply_sequence(gaussians, times, out_dir)              # export_perframe_3DGS.py: one static 3DGS PLY per time

A frame time between two baked timestamps is one extra launch (fdgs_state_blend: linear in every field, sign-aligned and renormalised
for the quaternions) or the nearer baked frame (`interp="nearest"`).  At a baked timestamp the image is bit for bit the one
`fdgs.render(...)` returns under `torch.no_grad()`.  No gradient flows through any of this.

Memory: 236 bytes per Gaussian and timestamp with all five heads on (59 floats), 40 bytes with the dnerf / hypernerf defaults (no_do,
no_dshs: opacity and SH do not change with time and are stored once); `bake_bytes` is the exact figure, `bake(..., max_bytes=)` refuses
before it allocates.

Where much of the set hardly moves, `bake_sparse(gaussians, times, tol)` keeps ONE full state and per timestamp only the rows whose baked
values leave a tolerance band around their values at times[0]; `motion_extent` reports per row how far they go, `sparse_bake_bytes` is
the exact stored size.  `SparseBaked.render` has the contract of `Baked.render`; a frame at a new time is one fdgs_state_scatter launch
over the dynamic rows.

`render_motion` (Baked, SparseBaked, compose.Composite) is `render` plus per-pixel motion vectors toward another frame and the accumulated
alpha, for one extra blend pass over the frame's own sorted lists (csrc/motion.hip):

    out = baked.render_motion(cam, pipe, background, toward=previous_cam)     # out["motion"] [2,H,W] pixels, out["alpha"] [1,H,W]

`render_pick` (the same three classes) is `render` plus what is under every pixel -- the row of the Gaussian that dominates it, and the
row and view depth of the one at which the pixel turns opaque -- for one extra walk over those lists (csrc/render.hip: render_pick_kernel);
`unproject` takes a pixel and that depth to a world point:

    out = baked.render_pick(cam, pipe, background)                            # out["pick_id"], out["surface_id"] [H,W]; out["surface_depth"] [1,H,W]
    point = fdgs.playback.unproject(cam, torch.tensor([[x, y]]), out["surface_depth"][0, y, x].reshape(1))

`render_contrib` (the same three classes) answers the inverse question -- how much every ROW adds to the image: per row the sum and the
maximum of its blend weight over the pixels (optionally weighted by a [H,W] image: a lasso, a mask) and the pixels and tiles that show it,
accumulated over any number of views and times into a `Contribution` (csrc/render.hip: render_contrib_kernel).  `contribution` loops it
over cameras, `Baked.select_rows` drops what is never seen:

    seen = fdgs.playback.contribution(baked, cameras, pipe, background)       # seen.weight_sum / weight_max / pixels / tiles [N]
    small = baked.select_rows(seen.keep_mask(min_pixels=1))                   # the same images from those views, fewer bytes
    inside = baked.render_contrib(cam, pipe, background, pixel_weight=lasso)["contribution"].pixels > 0

`render_features` (the same three classes) blends C per-row channels of the caller's -- a per-model indicator, `motion_extent`, a
`Contribution` column, labels, normals, embeddings -- like a colour, all C in one extra walk over those lists and without touching the
frame's colours (csrc/render.hip: render_features_kernel):

    out = baked.render_features(cam, pipe, background, seen.weight_sum)       # out["features"] [C,H,W], out["alpha"] [1,H,W]
    mattes = scene.render_features(cam, pipe, background, scene.model_indicator())["features"]       # one matte per placed model
"""
import bisect
import math
import os

import torch

from . import _lib
from . import deformation as _deformation
from . import io as _io
from . import rasterizer as _rasterizer
from . import renderer as _renderer

FIELDS = ("xyz", "scales", "rotations", "opacity", "shs")          # in the order of deformation.HEAD_NAMES: head h moves field h
FIELD_WIDTH = _deformation.HEAD_K                                   # floats per Gaussian: 3, 3, 4, 1, 48
FIELD_SHAPE = ((3,), (3,), (4,), (1,), (16, 3))
# every stored array starts on a multiple of this many floats (256 bytes, what the allocator gives a tensor of its own; fdgs_state_blend
# needs 16 bytes): the slot stride is padded, N * width is never assumed to be a multiple of anything
SLOT_ALIGN_FLOATS = 64


def _carve(slots, buf=None):
    """THE slot layout: `slots`, a sequence of (rows, row shape, copies), laid out back to back in a flat float32 buffer, every array
    starting on a multiple of SLOT_ALIGN_FLOATS -> (floats needed, per slot the list of its `copies` [rows, *shape] views of `buf`).
    Without a buffer it only counts, which is how the *_bytes functions and the allocations agree."""
    off, views = 0, []
    for rows, shape, copies in slots:
        n = rows * math.prod(shape)
        stride = (n + SLOT_ALIGN_FLOATS - 1) // SLOT_ALIGN_FLOATS * SLOT_ALIGN_FLOATS
        if buf is not None:
            views.append([buf[off + k * stride:off + k * stride + n].view(rows, *shape) for k in range(copies)])
        off += stride * copies
    return off, views


def _field_slots(N, copies=(1,) * len(FIELDS)):
    """One slot per field of FIELDS for _carve: [N, *FIELD_SHAPE[h]], copies[h] times (0: no floats, an empty list of views)."""
    return [(N, shape, c) for shape, c in zip(FIELD_SHAPE, copies)]


def _field_mask(head_on):
    """Bit h set for every field whose head is on: the `mask` of the fdgs_state_* calls."""
    return sum(1 << h for h, on in enumerate(head_on) if on)


def bake_bytes(N, T, head_on):
    """Bytes `bake` stores for N Gaussians and T timestamps: a field whose head is on (`head_on[h]`, the order of FIELDS: positions, scales,
    rotations, opacity, SH) takes one padded slot per timestamp, a field whose head is off one slot in all."""
    if N < 0 or T < 1 or len(head_on) != len(FIELDS):
        raise ValueError("bake_bytes: N >= 0, T >= 1 and one flag per field")
    return 4 * _carve(_field_slots(N, [T if on else 1 for on in head_on]))[0]


def _checked_times(times):
    ts = [float(t) for t in times]
    if not ts:
        raise ValueError("times: at least one timestamp")
    if any(math.isnan(t) or math.isinf(t) for t in ts) or any(b <= a for a, b in zip(ts, ts[1:])):
        raise ValueError("times: a strictly increasing sequence of finite floats")
    return ts


def _checked_interp(interp):
    if interp not in ("linear", "nearest"):
        raise ValueError(f"interp: 'linear' or 'nearest', not {interp!r}")
    return interp


def _locate(ts, t, interp):
    t = min(max(float(t), ts[0]), ts[-1])
    j = bisect.bisect_left(ts, t)                  # the first timestamp >= t
    if ts[j] == t:
        return j, j, 0.0
    i = j - 1
    if interp == "linear":
        return i, j, (t - ts[i]) / (ts[j] - ts[i])
    k = i if t - ts[i] <= ts[j] - t else j         # a tie goes to the lower index
    return k, k, 0.0


def locate(times, t, interp="linear"):
    """Where frame time `t` falls in the strictly increasing `times` (pure Python, float64): (i, j, w) such that the state at t is
    state_i + w * (state_j - state_i).  t is clamped to [times[0], times[-1]]; t == times[i] gives (i, i, 0.0); interp="linear" gives the
    bracketing pair and w = (t - t_i) / (t_j - t_i); interp="nearest" gives (k, k, 0.0) for the nearer timestamp, the lower one on a tie."""
    return _locate(_checked_times(times), t, _checked_interp(interp))


def to_rgb8(image, mode="trunc"):
    """float32 [3,H,W] device image -> uint8 [H,W,3] device tensor (fdgs_image_rgb8).  mode "trunc" is the reference's to8b,
    (255 * clip(x, 0, 1)).astype(uint8); "round" is what torchvision.utils.save_image stores, x * 255 + 0.5 clamped to [0, 255] and
    truncated.  NaN pixels are unspecified."""
    if mode not in _lib.RGB8_MODES:
        raise ValueError(f"mode: 'trunc' or 'round', not {mode!r}")
    if image.dim() != 3 or image.shape[0] != 3 or image.dtype != torch.float32:
        raise ValueError("to_rgb8: a float32 [3,H,W] image")
    if not _deformation._is_hip_device(image.device):
        raise _lib.FdgsError("to_rgb8 runs on the GPU only")
    img = image.detach().contiguous()
    H, W = int(img.shape[1]), int(img.shape[2])
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=img.device)
    _lib.check(_lib.lib().fdgs_image_rgb8(_lib.stream_ptr(), H, W, _lib.RGB8_MODES[mode], _lib.ptr(img), _lib.ptr(out)))
    return out


class BakedFrame:
    """The five arrays of one timestamp, views into the storage of their `Baked`.  The arrays of a head that is off are the SAME tensors in
    every frame."""
    __slots__ = FIELDS

    def __init__(self, arrays):
        for name, a in zip(FIELDS, arrays):
            setattr(self, name, a)

    def arrays(self):
        return (self.xyz, self.scales, self.rotations, self.opacity, self.shs)


def _perm_maps(perm):
    """The two row maps of _render_state for rows stored through `perm`: (model order -> stored order, stored order -> model order)."""
    if perm is None:
        return None, None
    return (lambda t: _deformation.permute_rows(perm, [t])[0]), (lambda t: _deformation.permute_rows(perm, [t], scatter=True)[0])


def _render_state(who, frame_at, sh_degree, device, to_stored, to_model, viewpoint_camera, pipe, bg_color, scaling_modifier, override_color,
                  cam_type, rgb8):
    """The body of Baked.render, SparseBaked.render and Composite.render: the rasterizer on the BakedFrame `frame_at(frame time)`.
    `to_stored` / `to_model` (None: the rows are stored in the model's order) take `override_color` to the stored row order and bring
    `radii` back.
    The camera's time is taken as a number, here and in every other playback render* method (render_motion, render_pick, render_contrib,
    render_features): a baked state has no deformation to differentiate, so a time tensor that requires grad gets its gradient from
    fdgs.render of the live model (fdgs.camera.TimeDelta), not from a playback frame."""
    if pipe.compute_cov3D_python or pipe.convert_SHs_python:
        raise NotImplementedError(f"{who}: pipe.compute_cov3D_python / pipe.convert_SHs_python need the live model; use fdgs.render")
    with torch.no_grad():
        raster_settings, frame_time = _renderer._frame_settings(viewpoint_camera, cam_type, bg_color, scaling_modifier, sh_degree, device, pipe)
        return _state_frame(frame_at(frame_time), raster_settings, to_stored, to_model, override_color, rgb8, pipe)[0]


def _state_frame(st, raster_settings, to_stored, to_model, override_color, rgb8, pipe=None):
    """(result dict, RasterState) of the forward-only frame of the BakedFrame `st`: what _render_state returns, and what it leaves behind.
    `pipe.antialiasing`: the frame is projected with the opacity compensation, as render() projects it (the replay passes read the state)."""
    shs, colors = st.shs, None
    if override_color is not None:
        shs, colors = None, override_color.detach().float()
        if to_stored is not None:
            colors = to_stored(colors)
    opts = _rasterizer.FrameOptions.of(pipe)._replace(alpha=False, absgrad=False)       # (a playback frame takes the projection's option only)
    image, radii, depth, rstate = _rasterizer.rasterize_forward(raster_settings, st.xyz, shs, colors, st.opacity, st.scales, st.rotations,
                                                                None, expect_backward=False, **opts.keywords())
    vis = rstate.visibility
    if to_model is not None:
        radii = to_model(radii)
        vis = radii > 0
    out = {"render": image, "viewspace_points": None, "visibility_filter": vis, "radii": radii, "depth": depth}
    if rgb8 is not None:
        out["rgb8"] = to_rgb8(image, rgb8)
    return out, rstate


def _render_motion_state(who, owner, frame_at, sh_degree, device, to_stored, to_model, viewpoint_camera, pipe, bg_color, toward, toward_time,
                         scaling_modifier, cam_type, min_alpha, rgb8):
    """The body of Baked.render_motion, SparseBaked.render_motion and Composite.render_motion: the frame of _render_state, then ONE more
    blend over the frame's own sorted lists with the per-row screen-space motion as the colour (include/fdgs.h at fdgs_geom_field: recC may
    be rewritten between two fdgs_render_fwd calls of a forward-only frame), then the per-pixel resolve.  `owner` keeps the [N,3] copy of
    the toward positions and the three zeros of the second blend's background (allocated on first use, not counted in nbytes)."""
    if toward is None and toward_time is None:
        raise ValueError(f"{who}: give `toward` (a camera: its pose and its time), `toward_time`, or both")
    if pipe.compute_cov3D_python or pipe.convert_SHs_python:
        raise NotImplementedError(f"{who}: pipe.compute_cov3D_python / pipe.convert_SHs_python need the live model; use fdgs.render")
    with torch.no_grad():
        raster_settings, frame_time = _renderer._frame_settings(viewpoint_camera, cam_type, bg_color, scaling_modifier, sh_degree, device, pipe)
        to_settings, t_to = raster_settings, frame_time
        if toward is not None:
            to_settings, t_to = _renderer._frame_settings(toward, cam_type, bg_color, scaling_modifier, sh_degree, device, pipe)
            if (int(to_settings.image_width), int(to_settings.image_height)) != (int(raster_settings.image_width), int(raster_settings.image_height)):
                raise ValueError(f"{who}: the `toward` camera must have the image size of the frame's camera")
        if toward_time is not None:
            t_to = float(toward_time)
        L = _lib.lib()
        N = owner.N
        if owner._motion_bufs is None:
            owner._motion_bufs = (torch.empty(N, 3, dtype=torch.float32, device=device), torch.zeros(3, dtype=torch.float32, device=device))
        xyz_to, zero_bg = owner._motion_bufs
        xyz_to.copy_(frame_at(t_to).xyz)          # (the next state_at may overwrite the scratch / working state this one lives in)
        st = frame_at(frame_time)
        out, rstate = _state_frame(st, raster_settings, to_stored, to_model, None, rgb8, pipe)
        p = rstate.params
        W, H = int(p.W), int(p.H)
        view_at, proj_at = rstate.keep[8], rstate.keep[9]
        view_to, proj_to = _rasterizer._f32(to_settings.viewmatrix, device), _rasterizer._f32(to_settings.projmatrix, device)
        recC = _lib.c_void_p()
        _lib.check(L.fdgs_geom_field(_lib.ptr(rstate.geom), N, 3, recC))
        stream = _lib.stream_ptr()
        _lib.check(L.fdgs_motion_rows(stream, N, _lib.ptr(st.xyz), _lib.ptr(xyz_to), _lib.ptr(view_at), _lib.ptr(proj_at), _lib.ptr(view_to),
                                      _lib.ptr(proj_to), W, H, recC, 4))
        p2 = _lib.RasterParams.from_buffer_copy(p)
        p2.bg, p2.acc_zero = _lib.ptr(zero_bg), None
        raw = torch.empty(3, H, W, dtype=torch.float32, device=device)
        # (depth does not depend on colour: the second blend writes the frame's depth over itself)
        _lib.check(L.fdgs_render_fwd(stream, p2, _lib.ptr(rstate.geom), _lib.ptr(rstate.binning), _lib.ptr(rstate.img), rstate.capacity,
                                     _lib.ptr(raw), _lib.ptr(out["depth"])))
        motion = torch.empty(2, H, W, dtype=torch.float32, device=device)
        alpha = torch.empty(1, H, W, dtype=torch.float32, device=device)
        _lib.check(L.fdgs_motion_resolve(stream, H, W, float(min_alpha), _lib.ptr(raw), _lib.ptr(motion), _lib.ptr(alpha)))
        out["motion_raw"], out["motion"], out["alpha"] = raw, motion, alpha
        return out


_MOTION_DOC = """Everything `render(viewpoint_camera, pipe, bg_color, scaling_modifier, cam_type=cam_type, interp=interp, rgb8=rgb8)` returns,
        bit for bit, plus per-pixel motion vectors and coverage at the cost of ONE extra blend pass (no second projection or sort):
          "motion_raw" [3,H,W]  the blend of (mx, my, 1) per Gaussian over a zero background,
          "motion"     [2,H,W]  motion_raw[:2] / motion_raw[2] where that is > min_alpha, else 0: ADD it to a pixel's coordinates in this
                                frame to find the same surface point in the toward frame (pixels),
          "alpha"      [1,H,W]  the accumulated alpha (1 - final_T), a copy of motion_raw[2].
        `toward`: a camera of the same kind as `viewpoint_camera` -- its pose and its time are used (None: the same pose); `toward_time`
        overrides the time.  At least one of the two, or ValueError; a `toward` camera of another image size: ValueError.  Times are clamped
        and located as `render` locates them.  A Gaussian behind the near plane (view depth <= 0.2) of EITHER camera contributes (0, 0, 1)."""


def _perm_row_map(perm):
    """The stored -> model row map of rows stored through `perm` (stored row i is model row perm[i]) as the int32 tensor fdgs_render_pick
    reads, or None for rows stored in the model's order."""
    return None if perm is None else perm.to(torch.int32).contiguous()


def _render_pick_state(who, owner, frame_at, sh_degree, device, to_stored, to_model, viewpoint_camera, pipe, bg_color, scaling_modifier,
                       cam_type, alpha_cut, rgb8):
    """The body of Baked.render_pick, SparseBaked.render_pick and Composite.render_pick: the frame of _render_state, then ONE
    fdgs_render_pick over the RasterState it left behind (include/fdgs.h: one more walk over the frame's own sorted lists, which writes
    nothing into them).  `owner` keeps the stored -> model row map (built on first use, not counted in nbytes)."""
    if pipe.compute_cov3D_python or pipe.convert_SHs_python:
        raise NotImplementedError(f"{who}: pipe.compute_cov3D_python / pipe.convert_SHs_python need the live model; use fdgs.render")
    alpha_cut = float(alpha_cut)
    if not 0.0 < alpha_cut <= 1.0:
        raise ValueError(f"{who}: alpha_cut in (0, 1], not {alpha_cut!r}")
    with torch.no_grad():
        raster_settings, frame_time = _renderer._frame_settings(viewpoint_camera, cam_type, bg_color, scaling_modifier, sh_degree, device, pipe)
        if owner._pick_row_map is None:          # (stays None for rows stored in the model's order: there is nothing to build)
            owner._pick_row_map = owner._make_pick_row_map()
        row_map = owner._pick_row_map
        out, rstate = _state_frame(frame_at(frame_time), raster_settings, to_stored, to_model, None, rgb8, pipe)
        p = rstate.params
        W, H = int(p.W), int(p.H)
        ids = torch.empty(2, H, W, dtype=torch.int32, device=device)
        vals = torch.empty(2, H, W, dtype=torch.float32, device=device)
        po = _lib.PickOut()
        po.pick_id, po.surface_id, po.pick_weight, po.surface_depth = ids[0].data_ptr(), ids[1].data_ptr(), vals[0].data_ptr(), vals[1].data_ptr()
        _lib.check(_lib.lib().fdgs_render_pick(_lib.stream_ptr(), p, _lib.ptr(rstate.geom), _lib.ptr(rstate.binning), _lib.ptr(rstate.img),
                                               rstate.capacity, alpha_cut, _lib.ptr(row_map), po))
        out["pick_id"], out["surface_id"], out["pick_weight"], out["surface_depth"] = ids[0], ids[1], vals[0], vals[1:2]
        return out


_PICK_DOC = """Everything `render(viewpoint_camera, pipe, bg_color, scaling_modifier, cam_type=cam_type, interp=interp, rgb8=rgb8)` returns,
        bit for bit, plus what is under every pixel, at the cost of ONE extra walk over the frame's own sorted lists (fdgs_render_pick: no
        second projection, sort or blend):
          "pick_id"       int32   [H,W]    the row of the Gaussian with the largest blend weight w = alpha * T at the pixel (on a tie the
                                           one in front); -1 where nothing contributed,
          "pick_weight"   float32 [H,W]    that weight, the bits the frame blended the Gaussian's colour with; 0 where nothing contributed,
          "surface_id"    int32   [H,W]    the row of the first Gaussian, front to back, with which the accumulated alpha reaches
                                           `alpha_cut`; -1 where it never does,
          "surface_depth" float32 [1,H,W]  that Gaussian's view depth (alpha_cut = 0.5: the median depth, a depth that lies ON a surface,
                                           where "depth" is the alpha-weighted mean); 0 where surface_id is -1.
        The ids follow the row order of "radii".  alpha_cut outside (0, 1]: ValueError.  `unproject` turns a pixel and its surface_depth
        into a world point."""


def unproject(viewpoint_camera, xy, depth, cam_type=None):
    """World points [K,3] of the pixel coordinates `xy` [K,2] (x = column, y = row; fractions allowed) at the view depths `depth` [K], in
    the rasterizer's pixel convention: ndc = (2 * px + 1) / W - 1, x_view = ndc_x * tanfovx * z, y_view = ndc_y * tanfovy * z, then the
    inverse of the view matrix.  Plain torch ops on the device of `depth`; with "surface_depth" of render_pick a click becomes the point to
    place a model at.  `viewpoint_camera`: a camera as `render` takes it (the PanopticSports dict with cam_type="PanopticSports")."""
    if cam_type == "PanopticSports":
        s = viewpoint_camera["camera"]
        W, H, tanx, tany, view = int(s.image_width), int(s.image_height), float(s.tanfovx), float(s.tanfovy), s.viewmatrix
    else:
        W, H = int(viewpoint_camera.image_width), int(viewpoint_camera.image_height)
        tanx, tany = math.tan(viewpoint_camera.FoVx * 0.5), math.tan(viewpoint_camera.FoVy * 0.5)
        view = viewpoint_camera.world_view_transform
    with torch.no_grad():
        z = depth.detach().reshape(-1).float()
        xy = xy.detach().reshape(-1, 2).to(device=z.device, dtype=torch.float32)
        if xy.shape[0] != z.shape[0]:
            raise ValueError("unproject: xy [K,2] and depth [K]")
        view = view.detach().to(device=z.device, dtype=torch.float32)
        nx = (2.0 * xy[:, 0] + 1.0) / W - 1.0
        ny = (2.0 * xy[:, 1] + 1.0) / H - 1.0
        pv = torch.stack([nx * tanx * z, ny * tany * z, z, torch.ones_like(z)], dim=1)
        return (pv @ torch.linalg.inv(view))[:, :3]          # (row vectors: p_view = [p_world, 1] @ view, the rasterizer's layout)


class Contribution:
    """Per-row blend weight statistics accumulated over any number of `render_contrib` passes (views, times): ONE zeroed [N,4] int32
    buffer of fdgs_contrib_row records, `rows`, and views of its columns --
      weight_sum  float32 [N]  sum over the passes' pixels of v = w * pixel_weight (w = alpha * T, the weight the frame blended the
                               row's colour with); float32 additions in no fixed order,
      weight_max  float32 [N]  the largest v of any pixel of any pass (exact),
      pixels      int32   [N]  pixels with v > 0, summed over the passes (exact),
      tiles       int32   [N]  16 x 16 tiles holding such a pixel, summed over the passes (exact),
    and `frames`, the host's count of the passes accumulated.  Rows are in the order of "radii"."""

    def __init__(self, N, device):
        self.N = int(N)
        if self.N < 0:
            raise ValueError("Contribution: N >= 0")
        self.rows = torch.zeros(self.N, 4, dtype=torch.int32, device=device)
        self.frames = 0

    @property
    def device(self):
        return self.rows.device

    @property
    def weight_sum(self):
        return self.rows[:, 0].view(torch.float32)

    @property
    def weight_max(self):
        return self.rows[:, 1].view(torch.float32)

    @property
    def pixels(self):
        return self.rows[:, 2]

    @property
    def tiles(self):
        return self.rows[:, 3]

    def reset(self):
        self.rows.zero_()
        self.frames = 0

    def keep_mask(self, min_pixels=1, min_weight_max=0.0, min_weight_sum=0.0):
        """bool [N]: the rows that reach all three thresholds (pixels >= min_pixels, weight_max >= min_weight_max, weight_sum >=
        min_weight_sum).  The default keeps what was blended into at least one pixel: the mask `Baked.select_rows` takes."""
        return (self.pixels >= int(min_pixels)) & (self.weight_max >= float(min_weight_max)) & (self.weight_sum >= float(min_weight_sum))


def _render_contrib_state(who, owner, frame_at, sh_degree, device, to_stored, to_model, viewpoint_camera, pipe, bg_color, into, pixel_weight,
                          scaling_modifier, cam_type, rgb8):
    """The body of Baked.render_contrib, SparseBaked.render_contrib and Composite.render_contrib: the frame of _render_state, then ONE
    fdgs_render_contrib over the RasterState it left behind (include/fdgs.h: one more walk over the frame's own sorted lists, which writes
    nothing into them), accumulated through the owner's stored -> model row map into `into`."""
    if pipe.compute_cov3D_python or pipe.convert_SHs_python:
        raise NotImplementedError(f"{who}: pipe.compute_cov3D_python / pipe.convert_SHs_python need the live model; use fdgs.render")
    with torch.no_grad():
        raster_settings, frame_time = _renderer._frame_settings(viewpoint_camera, cam_type, bg_color, scaling_modifier, sh_degree, device, pipe)
        W, H = int(raster_settings.image_width), int(raster_settings.image_height)
        if into is None:
            into = Contribution(owner.N, device)
        elif not isinstance(into, Contribution) or into.N != owner.N or into.device != device:
            raise ValueError(f"{who}: `into` must be a Contribution of {owner.N} rows on {device}")
        if pixel_weight is not None:
            if (not torch.is_tensor(pixel_weight) or pixel_weight.dtype != torch.float32 or pixel_weight.device != device
                    or tuple(pixel_weight.shape) not in ((H, W), (1, H, W))):
                raise ValueError(f"{who}: pixel_weight must be a float32 [{H},{W}] or [1,{H},{W}] tensor on {device}")
            pixel_weight = pixel_weight.detach().contiguous()
        if owner._pick_row_map is None:          # (stays None for rows stored in the model's order: there is nothing to build)
            owner._pick_row_map = owner._make_pick_row_map()
        out, rstate = _state_frame(frame_at(frame_time), raster_settings, to_stored, to_model, None, rgb8, pipe)
        if into.N > 0:
            _lib.check(_lib.lib().fdgs_render_contrib(_lib.stream_ptr(), rstate.params, _lib.ptr(rstate.geom), _lib.ptr(rstate.binning),
                                                      _lib.ptr(rstate.img), rstate.capacity, _lib.ptr(pixel_weight),
                                                      _lib.ptr(owner._pick_row_map), _lib.ptr(into.rows)))
        into.frames += 1
        out["contribution"] = into
        return out


_CONTRIB_DOC = """Everything `render(viewpoint_camera, pipe, bg_color, scaling_modifier, cam_type=cam_type, interp=interp, rgb8=rgb8)` returns,
        bit for bit, plus "contribution": how much every row adds to this image, ACCUMULATED into `into` (a `Contribution` of this
        object's N rows on its device; None: a new one), at the cost of ONE extra walk over the frame's own sorted lists
        (fdgs_render_contrib: no second projection, sort or blend).  Per row, over the frame's pixels: the sum and the maximum of
        v = w * pixel_weight (w = alpha * T, the weight the frame blended the row's colour with), the number of pixels with v > 0 and of
        the 16 x 16 tiles that hold one.  `pixel_weight`: a float32 [H,W] or [1,H,W] tensor on the device (a lasso, a mask, a saliency
        map; a pixel whose weight is zero, negative or NaN counts for nothing), None: 1 everywhere.  Rows follow the order of "radii".  A
        pixel_weight of another shape, dtype or device, or an `into` of another N or device: ValueError."""


def _checked_values(who, values, N, device):
    """`values` of render_features as the [N, C] view fdgs_render_features reads in place -> (view, C, floats from one row to the next)."""
    if (not torch.is_tensor(values) or values.dtype != torch.float32 or values.device != device or values.dim() not in (1, 2)
            or values.shape[0] != N or (values.dim() == 2 and values.shape[1] < 1)):
        raise ValueError(f"{who}: values must be a float32 [{N}] or [{N}, C] tensor (C >= 1) on {device}")
    v = values.detach()
    if v.dim() == 1:
        v = v.unsqueeze(1)
    C = int(v.shape[1])
    stride = int(v.stride(0)) if N > 1 else C          # (the stride of a dimension of size <= 1 means nothing)
    if (C > 1 and v.stride(1) != 1) or stride < C:
        raise ValueError(f"{who}: values must have stride 1 in its last dimension and rows that do not overlap (strides {tuple(values.stride())})")
    return v, C, stride


class _FeaturesFrame:
    """What the backward of a differentiable feature pass needs of its frame: the RasterState (geom, binning, img, capacity, params), the
    owner's row map (None: the model's order), the alpha image, whether and from which alpha on the forward normalised, and N, C.  Kept
    by the autograd graph of "features": a pending graph pins ONE frame's buffers, nothing else of the owner."""
    __slots__ = ("rstate", "row_map", "alpha", "normalize", "min_alpha", "N", "C", "features")


class _FeaturesOfValues(torch.autograd.Function):
    """"features" as a function of `values`: the forward hands out the image fdgs_render_features wrote (the plain pass's bits), the backward
    is ONE fdgs_render_features_bwd over the same frame's lists into a zeroed [N,C].  Nothing is consumed: a second backward of a retained
    graph runs the same call again.  Not differentiable twice; no gradient reaches the geometry."""

    @staticmethod
    def forward(ctx, values, frame):
        ctx.frame, ctx.values_shape = frame, tuple(values.shape)
        ctx.set_materialize_grads(False)
        features, frame.features = frame.features, None
        return features

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        if grad is None:
            return None, None
        f = ctx.frame
        rstate = f.rstate
        g = grad.to(torch.float32).contiguous()
        dvalues = torch.zeros(f.N, f.C, dtype=torch.float32, device=g.device)
        _lib.check(_lib.lib().fdgs_render_features_bwd(_lib.stream_ptr(), rstate.params, _lib.ptr(rstate.geom), _lib.ptr(rstate.binning),
                                                       _lib.ptr(rstate.img), rstate.capacity, f.C, _lib.ptr(g),
                                                       _lib.ptr(f.alpha) if f.normalize else None, f.min_alpha if f.normalize else -1.0,
                                                       _lib.ptr(f.row_map), f.N, _lib.ptr(dvalues), f.C))
        return dvalues.view(ctx.values_shape), None


def _render_features_state(who, owner, frame_at, sh_degree, device, to_stored, to_model, viewpoint_camera, pipe, bg_color, values, normalize,
                           min_alpha, scaling_modifier, cam_type, rgb8, differentiable=False):
    """The body of Baked.render_features, SparseBaked.render_features and Composite.render_features: the frame of _render_state, then ONE
    fdgs_render_features over the RasterState it left behind (include/fdgs.h: one more walk over the frame's own sorted lists, which writes
    nothing into them), reading `values` in place through the owner's stored -> model row map.  `differentiable` with grad mode on and
    values that require grad: the same calls, and "features" leaves through _FeaturesOfValues."""
    if pipe.compute_cov3D_python or pipe.convert_SHs_python:
        raise NotImplementedError(f"{who}: pipe.compute_cov3D_python / pipe.convert_SHs_python need the live model; use fdgs.render")
    v, C, stride = _checked_values(who, values, owner.N, device)
    min_alpha = float(min_alpha)
    if normalize and not min_alpha >= 0.0:
        raise ValueError(f"{who}: min_alpha >= 0 with normalize=True, not {min_alpha!r}")
    with torch.no_grad():
        raster_settings, frame_time = _renderer._frame_settings(viewpoint_camera, cam_type, bg_color, scaling_modifier, sh_degree, device, pipe)
        if owner._pick_row_map is None:          # (stays None for rows stored in the model's order: there is nothing to build)
            owner._pick_row_map = owner._make_pick_row_map()
        out, rstate = _state_frame(frame_at(frame_time), raster_settings, to_stored, to_model, None, rgb8, pipe)
        p = rstate.params
        W, H = int(p.W), int(p.H)
        if owner.N == 0:                          # (an empty tensor has no address to hand over)
            out["features"], out["alpha"] = torch.zeros(C, H, W, device=device), torch.zeros(1, H, W, device=device)
            return out
        features = torch.empty(C, H, W, dtype=torch.float32, device=device)
        alpha = torch.empty(1, H, W, dtype=torch.float32, device=device)
        _lib.check(_lib.lib().fdgs_render_features(_lib.stream_ptr(), p, _lib.ptr(rstate.geom), _lib.ptr(rstate.binning), _lib.ptr(rstate.img),
                                                   rstate.capacity, C, v.data_ptr(), stride, owner.N, _lib.ptr(owner._pick_row_map),
                                                   min_alpha if normalize else -1.0, _lib.ptr(features), _lib.ptr(alpha)))
        out["features"], out["alpha"] = features, alpha
    if differentiable and torch.is_grad_enabled() and values.requires_grad:
        f = _FeaturesFrame()
        f.rstate, f.row_map, f.alpha, f.normalize, f.min_alpha, f.N, f.C = rstate, owner._pick_row_map, alpha, bool(normalize), min_alpha, owner.N, C
        f.features = features
        out["features"] = _FeaturesOfValues.apply(values, f)
    return out


_FEATURES_DOC = """Everything `render(viewpoint_camera, pipe, bg_color, scaling_modifier, cam_type=cam_type, interp=interp, rgb8=rgb8)` returns,
        bit for bit, plus C per-row channels of the caller's blended like a colour, at the cost of ONE extra walk over the frame's own
        sorted lists for any C (fdgs_render_features: no second projection, sort or blend; the frame's colours are not touched):
          "features" float32 [C,H,W]  channel c = the sum over the pixel's contributors of values[row, c] * w, w = alpha * T the weight
                                      the frame blended the row's colour with: the bits `render(..., bg_color=0, override_color=values[:,
                                      c:c+3])["render"]` has for that channel.  No background is added.  With normalize=True: that sum
                                      divided by "alpha" where "alpha" > min_alpha, 0 elsewhere (the expected value of the channel over
                                      what the pixel shows: a label or an embedding that does not fade at the silhouette),
          "alpha"    float32 [1,H,W]  the accumulated alpha, the sum of w.
        `values`: a float32 [N] or [N,C] tensor on the device in the row order of "radii" (a per-model indicator, `motion_extent`, a
        `Contribution` column, labels, normals, embeddings); read in place -- it need not be contiguous as long as its last dimension
        has stride 1, e.g. a column slice of a wider array.  Anything else: ValueError.
        `differentiable=True`, with grad mode on and `values.requires_grad`: "features" (the same bits, from the same calls) carries the
        gradient to `values` -- d features[c, pixel] / d values[row, c] = w, or w / "alpha" where normalised --, computed by ONE
        fdgs_render_features_bwd over this frame's own lists per backward, in the shape of `values`; what a frozen model's per-row
        embeddings, labels or identities are fitted to 2-D masks and feature maps with.  Nothing else is differentiable: "alpha", every
        key of `render`, and the geometry behind the weights (the path through "alpha" of a normalised pass included).  The graph of
        "features" holds this frame's rasterizer buffers until it is freed -- a pending graph pins one frame's buffers --, and a
        backward may run after later frames were rendered, any number of times (retain_graph).  The gradient image must be finite.
        Otherwise (the default, no_grad, values without requires_grad): exactly the plain pass."""


class _AtTime:
    """`camera` with another frame time: every other attribute is the camera's own."""

    def __init__(self, camera, time):
        self._camera, self.time = camera, float(time)

    def __getattr__(self, name):
        return getattr(self._camera, name)


def contribution(obj, cameras, pipe, bg_color, times=None, **kw):
    """One `Contribution` accumulated over `cameras`: obj.render_contrib (a Baked, SparseBaked or Composite) once per camera at the
    camera's own time, or, when `times` is given, once per camera and time of `times`.  **kw goes to render_contrib (pixel_weight,
    scaling_modifier, cam_type, interp; `into` to go on accumulating into an existing one).  The importance statistic of a pruning pass:
    `baked.select_rows(contribution(baked, cams, pipe, bg).keep_mask())` drops what no view shows."""
    into = kw.pop("into", None)
    if into is None:
        into = Contribution(obj.N, obj.device)
    for cam in cameras:
        if times is None:
            obj.render_contrib(cam, pipe, bg_color, into=into, **kw)
            continue
        for t in times:
            at = {**cam, "time": float(t)} if kw.get("cam_type") == "PanopticSports" else _AtTime(cam, t)
            obj.render_contrib(at, pipe, bg_color, into=into, **kw)
    return into


class Baked:
    """The deformed, activated state of a model at `times`, resident on the device: positions [N,3], scales [N,3] (exp applied), rotations
    [N,4] (unit quaternions), opacity [N,1] (sigmoid applied), SH [N,16,3] -- what the no-grad branch of render() hands to the rasterizer.

    A SNAPSHOT: it holds copies, not references.  Training steps, densification, pruning, a reorder or a loaded checkpoint after `bake`
    leave it stale (it keeps rendering the model as it was); bake again.

    `times`, `frames[k]` (BakedFrame), `head_on`, `N`, `nbytes` (the stored size, == bake_bytes(N, len(times), head_on); the scratch state
    of the temporal blend, one more timestamp's worth of the time-dependent fields, is allocated on the first blended frame and not
    counted), `perm` (the implicit Hilbert permutation the rows are stored in, or None: rows in the model's order)."""

    def __init__(self, times, frames, head_on, perm, storage, active_sh_degree):
        self.times, self.frames, self.head_on, self.perm = tuple(times), frames, tuple(head_on), perm
        self._storage = storage
        self.active_sh_degree = active_sh_degree
        self.N = int(frames[0].xyz.shape[0])
        self.nbytes = storage.numel() * storage.element_size()
        self._scratch, self._maps = None, _perm_maps(perm)
        self._motion_bufs = None
        self._pick_row_map = None

    def _make_pick_row_map(self):
        return _perm_row_map(self.perm)

    @property
    def device(self):
        return self._storage.device

    def blend(self, i, j, w):
        """The state at weight `w` between frames i and j as a BakedFrame: ONE fdgs_state_blend launch into this object's scratch state
        (time-dependent fields only; the others are the stored arrays themselves).  The result is overwritten by the next blend."""
        if self._scratch is None:
            slots = _field_slots(self.N, [1 if on else 0 for on in self.head_on])
            buf = torch.empty(_carve(slots)[0], dtype=torch.float32, device=self.device)
            views = _carve(slots, buf)[1]
            self._scratch = (buf, BakedFrame([v[0] if v else static for v, static in zip(views, self.frames[0].arrays())]))
        out = self._scratch[1]
        a, b = self.frames[i], self.frames[j]
        streams = (_lib.BlendStream * _lib.MAX_BLEND_STREAMS)()
        ns = 0
        for h, name in enumerate(FIELDS):
            if self.head_on[h] and name != "rotations":
                s = streams[ns]
                s.a, s.b, s.out = getattr(a, name).data_ptr(), getattr(b, name).data_ptr(), getattr(out, name).data_ptr()
                s.n_floats = self.N * FIELD_WIDTH[h]
                ns += 1
        rot = (a.rotations, b.rotations, out.rotations) if self.head_on[2] else (None, None, None)
        _lib.check(_lib.lib().fdgs_state_blend(_lib.stream_ptr(), float(w), ns, streams, self.N, *[_lib.ptr(r) for r in rot]))
        return out

    def state_at(self, t, interp="linear"):
        """(BakedFrame, (i, j, w)) for frame time t: a stored frame when t is a baked timestamp (or interp="nearest"), else the blend."""
        i, j, w = _locate(self.times, t, _checked_interp(interp))
        if i == j or not any(self.head_on):
            return self.frames[i], (i, j, w)
        return self.blend(i, j, w), (i, j, w)

    def render(self, viewpoint_camera, pipe, bg_color, scaling_modifier=1.0, override_color=None, cam_type=None, interp="linear", rgb8=None):
        """`fdgs.render(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, override_color, "fine", cam_type)` under torch.no_grad(),
        with the deformation replaced by the baked state at the camera's time: the same raster settings (the PanopticSports dict camera
        included), the same result dict -- "viewspace_points" is None (nothing here takes a gradient), "radii" / "visibility_filter" are in
        the model's row order.  interp: what a time between two baked timestamps gets ("linear" | "nearest").  rgb8 = "trunc" | "round" adds
        "rgb8", the uint8 [H,W,3] image of to_rgb8.  The pipe's python SH / covariance paths are not available from a baked state.
        The camera's time is taken as a number (no gradient to a time tensor: that is fdgs.render's, on the live model)."""
        return _render_state("Baked.render", lambda t: self.state_at(t, interp)[0], self.active_sh_degree, self.device, *self._maps,
                             viewpoint_camera, pipe, bg_color, scaling_modifier, override_color, cam_type, rgb8)

    def render_motion(self, viewpoint_camera, pipe, bg_color, toward=None, toward_time=None, scaling_modifier=1.0, cam_type=None,
                      interp="linear", min_alpha=0.0, rgb8=None):
        return _render_motion_state("Baked.render_motion", self, lambda t: self.state_at(t, interp)[0], self.active_sh_degree, self.device,
                                    *self._maps, viewpoint_camera, pipe, bg_color, toward, toward_time, scaling_modifier, cam_type, min_alpha,
                                    rgb8)

    render_motion.__doc__ = _MOTION_DOC

    def render_pick(self, viewpoint_camera, pipe, bg_color, scaling_modifier=1.0, cam_type=None, interp="linear", alpha_cut=0.5, rgb8=None):
        return _render_pick_state("Baked.render_pick", self, lambda t: self.state_at(t, interp)[0], self.active_sh_degree, self.device,
                                  *self._maps, viewpoint_camera, pipe, bg_color, scaling_modifier, cam_type, alpha_cut, rgb8)

    render_pick.__doc__ = _PICK_DOC

    def render_contrib(self, viewpoint_camera, pipe, bg_color, into=None, pixel_weight=None, scaling_modifier=1.0, cam_type=None,
                       interp="linear", rgb8=None):
        return _render_contrib_state("Baked.render_contrib", self, lambda t: self.state_at(t, interp)[0], self.active_sh_degree, self.device,
                                     *self._maps, viewpoint_camera, pipe, bg_color, into, pixel_weight, scaling_modifier, cam_type, rgb8)

    render_contrib.__doc__ = _CONTRIB_DOC

    def render_features(self, viewpoint_camera, pipe, bg_color, values, normalize=False, min_alpha=1e-4, scaling_modifier=1.0, cam_type=None,
                        interp="linear", rgb8=None, differentiable=False):
        return _render_features_state("Baked.render_features", self, lambda t: self.state_at(t, interp)[0], self.active_sh_degree, self.device,
                                      *self._maps, viewpoint_camera, pipe, bg_color, values, normalize, min_alpha, scaling_modifier, cam_type,
                                      rgb8, differentiable)

    render_features.__doc__ = _FEATURES_DOC

    def select_rows(self, keep):
        """A new Baked holding only the rows `keep` selects -- a bool mask [N] or an integer index tensor, in the MODEL's row order (the
        order of "radii", of `Contribution.keep_mask`) --: the same times, head_on and active_sh_degree, arrays of a head that is off
        stored once, the layout of `bake` (nbytes == bake_bytes(N', T, head_on)).  A snapshot, like `bake`: it shares nothing with
        this object.  The STORED order is preserved: with `perm`, stored row i is kept iff keep[perm[i]], and the new `perm` maps the
        kept stored rows to the kept model rows renumbered ascending (new model row k is the k-th kept row of the old model).  Binning
        breaks depth ties by Gaussian index, so the subset sorts as it did inside the full set: dropping rows with pixels == 0 at a view
        leaves every pixel of that view's image and depth bit-identical that the frame did not END EARLY.  (The blend ends a pixel at the
        first entry with T * (1 - alpha) < 1e-4 WITHOUT blending that entry: a row that only ever ends pixels has pixels == 0, and
        without it such a pixel goes on to the next entry -- a change below the transmittance the pixel had left, < 0.01.  A view in
        which no pixel saturates is identical as a whole.)  A one-time operation in torch index ops, not a frame.  A mask of another
        length, or an index outside [0, N): ValueError.  (SparseBaked and Composite have no select_rows: select per model, then bake
        sparse or compose again.)"""
        keep = torch.as_tensor(keep, device=self.device)
        if keep.dtype == torch.bool:
            if tuple(keep.shape) != (self.N,):
                raise ValueError(f"Baked.select_rows: a bool mask of {self.N} rows, not {tuple(keep.shape)}")
            mask = keep
        else:
            if keep.dim() != 1 or keep.dtype.is_floating_point or keep.dtype.is_complex:
                raise ValueError("Baked.select_rows: a bool mask [N] or a 1-D integer index tensor")
            idx = keep.to(torch.int64)
            if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.N):
                raise ValueError(f"Baked.select_rows: an index outside [0, {self.N})")
            mask = torch.zeros(self.N, dtype=torch.bool, device=self.device)
            mask[idx] = True
        with torch.no_grad():
            stored_mask = mask if self.perm is None else mask[self.perm.to(torch.int64)]
            rows = torch.nonzero(stored_mask).reshape(-1)                 # the kept STORED rows, ascending: their order is preserved
            n, T = int(rows.numel()), len(self.times)
            perm = None
            if self.perm is not None:
                new_id = torch.cumsum(mask.to(torch.int64), 0) - 1          # old model row -> its rank among the kept model rows
                perm = new_id[self.perm.to(torch.int64)[rows]].to(self.perm.dtype).contiguous()
            storage = torch.empty(bake_bytes(n, T, self.head_on) // 4, dtype=torch.float32, device=self.device)
            views = _carve(_field_slots(n, [T if on else 1 for on in self.head_on]), storage)[1]
            slots = [v if on else v * T for v, on in zip(views, self.head_on)]
            for h, name in enumerate(FIELDS):
                for k in range(T if self.head_on[h] else 1):
                    slots[h][k].copy_(getattr(self.frames[k], name)[rows])
            frames = [BakedFrame([slots[h][k] for h in range(len(FIELDS))]) for k in range(T)]
        return Baked(self.times, frames, self.head_on, perm, storage, self.active_sh_degree)


def bake(pc, times, max_bytes=None):
    """Deforms `pc` once per timestamp and keeps the activated states on the device -> Baked.

    Per time: the deformation.forward_impl(..., activate=True) call of render()'s no-grad branch, on the same inputs -- read through the
    implicit Hilbert permutation when render() would read them through it (renderer._implicit_perm), so a baked frame rasterizes to the
    image render() gives, bit for bit.  Arrays of a head that is on are stored per timestamp, arrays of a head that is off once (from the
    first frame: they do not depend on the time).  Raises ValueError unless `times` is strictly increasing, MemoryError -- before anything
    is allocated -- when `max_bytes` is given and bake_bytes(...) exceeds it."""
    ts = _checked_times(times)
    head_on, N = _checked_model(pc, "bake")
    T = len(ts)
    need = bake_bytes(N, T, head_on)
    if max_bytes is not None and need > max_bytes:
        raise MemoryError(f"bake: {T} timestamps of {N} Gaussians need {need} bytes, max_bytes = {max_bytes}")
    with torch.no_grad():
        perm, forward = _deformer(pc)
        storage = torch.empty(need // 4, dtype=torch.float32, device=pc._xyz.device)
        # per field: the [N, ...] view of every timestamp (one shared view when the head is off)
        slots = [v if on else v * T for v, on in zip(_carve(_field_slots(N, [T if on else 1 for on in head_on]), storage)[1], head_on)]
        for k, t in enumerate(ts):
            for h, o in enumerate(forward(t)):
                if head_on[h] or k == 0:
                    slots[h][k].copy_(o)
        frames = [BakedFrame([slots[h][k] for h in range(len(FIELDS))]) for k in range(T)]
    return Baked(ts, frames, head_on, perm, storage, pc.active_sh_degree)


# ---- sparse bake: ONE full state, and per timestamp only the rows that move --------------------------------------------------------------

def _checked_tol(tol):
    try:
        vals = tuple(float(v) for v in tol)
    except TypeError:
        vals = (float(tol),) * len(FIELDS)
    if len(vals) != len(FIELDS):
        raise ValueError("tol: one float, or one per field in the order of FIELDS (positions, scales, rotations, opacity, SH)")
    if any(math.isnan(v) for v in vals):
        raise ValueError("tol: NaN is not a tolerance")
    return vals


def sparse_bake_bytes(N, D, T, head_on):
    """Bytes `bake_sparse` stores for N Gaussians of which D are dynamic, at T timestamps: one full state (all five fields, one padded slot
    each), per timestamp one padded [D, width] slot of every field whose head is on, and the int32 row list."""
    if N < 0 or T < 1 or not 0 <= D <= N or len(head_on) != len(FIELDS):
        raise ValueError("sparse_bake_bytes: N >= 0, 0 <= D <= N, T >= 1 and one flag per field")
    return 4 * (_carve(_field_slots(N))[0] + _carve(_compact_slots(D, T, head_on))[0])


def _compact_slots(D, T, head_on):
    """What bake_sparse keeps beside the full state: [D, ...] of every field whose head is on at every timestamp, then the D int32 rows."""
    return _field_slots(D, [T if on else 0 for on in head_on]) + [(D, (), 1)]


def _state_arrays(arrays, mask, row_offset=0):
    """fdgs_state_arrays over the five `arrays` from row `row_offset` on: the pointers of the fields `mask` selects, NULL elsewhere."""
    s = _lib.StateArrays()
    for h, name in enumerate(FIELDS):
        if mask >> h & 1:
            p = arrays[h].data_ptr()
            setattr(s, name, p + 4 * row_offset * FIELD_WIDTH[h] if row_offset else p)
    return s


def _deformer(pc):
    """(perm, forward): forward(t) is the five arrays render()'s no-grad branch hands to the rasterizer at time t -- its cfg, its implicit
    Hilbert permutation of the inputs (renderer._fine_stage), activate=True.  Call under torch.no_grad()."""
    cfg, perm, ins, net_ins = _renderer._fine_stage(pc)

    def forward(t):
        st = _deformation.forward_impl(cfg, t, *ins, None, net_ins[0], net_ins[1:], False)
        return (st.o_xyz, st.o_sc, st.o_rot, st.o_op, st.o_sh)
    return perm, forward


def _extent_pass(forward, ts, head_on, N, device):
    """(state at ts[0], extent [N,5] in the stored row order): one forward per timestamp, one fdgs_state_extent launch for each but the
    first.  Two states are alive at a time."""
    ref = forward(ts[0])
    ext = torch.zeros(N, len(FIELDS), dtype=torch.float32, device=device)
    mask = _field_mask(head_on)
    for t in ts[1:]:
        cur = forward(t)
        _lib.check(_lib.lib().fdgs_state_extent(_lib.stream_ptr(), N, mask, _state_arrays(ref, mask), _state_arrays(cur, mask), _lib.ptr(ext)))
    return ref, ext


def _checked_model(pc, who):
    net = pc._deformation
    if not isinstance(net, _deformation.deform_network):
        raise TypeError(f"{who}: pc._deformation must be this package's deform_network")
    return _deformation._head_on(net.deformation_net.args), int(pc._xyz.shape[0])


def motion_extent(pc, times):
    """How far every Gaussian's baked state gets from its state at times[0] -> float32 [N,5] on the model's device, rows in the MODEL's
    order: column h is the maximum, over the timestamps and the components of field h (the order of FIELDS), of |state_k - state_0| taken
    as one float32 subtraction (fdgs_state_extent); 0 where head h is off; +inf where a difference is a NaN.  What `bake_sparse` compares
    with `tol`: a quantile of a column is the tolerance that keeps that share of the rows static.  One deformation forward per timestamp,
    exactly `bake`'s; two states of scratch, whatever len(times)."""
    ts = _checked_times(times)
    head_on, N = _checked_model(pc, "motion_extent")
    with torch.no_grad():
        perm, forward = _deformer(pc)
        _, ext = _extent_pass(forward, ts, head_on, N, pc._xyz.device)
        if perm is not None:
            ext, = _deformation.permute_rows(perm, [ext], scatter=True)
    return ext


class SparseBaked:
    """A baked sequence that keeps ONE full working state and, per timestamp, only the DYNAMIC rows: row n is dynamic iff for some head h
    that is on motion_extent[n, h] > tol[h].  Stored bytes and the per-frame state update scale with D, the number of dynamic rows.

    What a frame holds (`state_at`, `render`), against the dense `Baked` of the same model and times:
      1. a dynamic row: at a baked timestamp the bits of the dense frame, at a time in between the bits `Baked.blend` gives that row;
      2. a static row: the bits of the dense frame at times[0], at every time.  At every baked timestamp each of its components is
         therefore within tol[h] of the dense frame (the difference taken as one float32 subtraction); between timestamps the linear fields
         stay within that band up to rounding; the renormalised quaternion blend has no such bound, but a row whose rotation leaves the
         band is dynamic anyway;
      3. tol < 0: D == N and every frame, baked or blended, is bit for bit Baked.render's (image, depth, radii, visibility);
      4. tol = inf: D == 0 and every frame is the frame at times[0], without a launch.

    A SNAPSHOT like `Baked`.  `times`, `head_on`, `N`, `D`, `rows` (int32 [D], ascending, in the stored row order), `dynamic` (bool [N], the
    model's row order), `perm` (the implicit Hilbert permutation the rows are stored in, or None), `tol` (5-tuple), `nbytes`
    (== sparse_bake_bytes(N, D, len(times), head_on)), `active_sh_degree`, `launches` (fdgs_state_scatter launches so far), `device`."""

    def __init__(self, times, head_on, perm, tol, working, arrays, compact_storage, compact, rows, dynamic, active_sh_degree):
        self.times, self.head_on, self.perm, self.tol = tuple(times), tuple(head_on), perm, tuple(tol)
        self._working, self._compact_storage, self._compact = working, compact_storage, compact
        self.rows, self.dynamic = rows, dynamic
        self.active_sh_degree = active_sh_degree
        self.N, self.D = int(arrays[0].shape[0]), int(rows.shape[0])
        self.nbytes = 4 * (working.numel() + compact_storage.numel())
        self.launches = 0
        self._mask = _field_mask(self.head_on)
        self._frame = BakedFrame(arrays)
        # the fdgs_state_arrays of every timestamp's compact rows and of the working state: they never change, filled once
        self._sources, self._target = [_state_arrays(c, self._mask) for c in compact], _state_arrays(arrays, self._mask)
        self._maps = _perm_maps(perm)
        self._shown = (0, 0, 0.0)               # the (i, j, w) the dynamic rows of the working state hold
        self._motion_bufs = None
        self._pick_row_map = None

    def _make_pick_row_map(self):
        return _perm_row_map(self.perm)

    @property
    def device(self):
        return self._working.device

    def state_at(self, t, interp="linear"):
        """(BakedFrame over the working state, (i, j, w)) for frame time t.  ONE fdgs_state_scatter launch (a copy of compact[i] at a baked
        timestamp or with interp="nearest", else the blend of compact[i] and compact[j] fused into it) when (i, j, w) is not what the
        working state holds; none when it is, when D == 0 or when no head is on.  The frame is overwritten by the next call."""
        key = _locate(self.times, t, _checked_interp(interp))
        if self.D and self._mask and key != self._shown:
            i, j, w = key
            blend = i != j
            _lib.check(_lib.lib().fdgs_state_scatter(_lib.stream_ptr(), self.D, _lib.ptr(self.rows), self.N, self._mask, self._sources[i],
                                                     self._sources[j] if blend else None, float(w) if blend else 0.0, self._target))
            self.launches += 1
            self._shown = key
        return self._frame, key

    def render(self, viewpoint_camera, pipe, bg_color, scaling_modifier=1.0, override_color=None, cam_type=None, interp="linear", rgb8=None):
        """The contract of `Baked.render`, on the state `state_at` gives."""
        return _render_state("SparseBaked.render", lambda t: self.state_at(t, interp)[0], self.active_sh_degree, self.device,
                             *self._maps, viewpoint_camera, pipe, bg_color, scaling_modifier, override_color, cam_type, rgb8)

    def render_motion(self, viewpoint_camera, pipe, bg_color, toward=None, toward_time=None, scaling_modifier=1.0, cam_type=None,
                      interp="linear", min_alpha=0.0, rgb8=None):
        return _render_motion_state("SparseBaked.render_motion", self, lambda t: self.state_at(t, interp)[0], self.active_sh_degree,
                                    self.device, *self._maps, viewpoint_camera, pipe, bg_color, toward, toward_time, scaling_modifier,
                                    cam_type, min_alpha, rgb8)

    render_motion.__doc__ = _MOTION_DOC + """
        Two state_at calls: up to two fdgs_state_scatter launches; the working state ends at the frame's time, as after `render`."""

    def render_pick(self, viewpoint_camera, pipe, bg_color, scaling_modifier=1.0, cam_type=None, interp="linear", alpha_cut=0.5, rgb8=None):
        return _render_pick_state("SparseBaked.render_pick", self, lambda t: self.state_at(t, interp)[0], self.active_sh_degree, self.device,
                                  *self._maps, viewpoint_camera, pipe, bg_color, scaling_modifier, cam_type, alpha_cut, rgb8)

    render_pick.__doc__ = _PICK_DOC

    def render_contrib(self, viewpoint_camera, pipe, bg_color, into=None, pixel_weight=None, scaling_modifier=1.0, cam_type=None,
                       interp="linear", rgb8=None):
        return _render_contrib_state("SparseBaked.render_contrib", self, lambda t: self.state_at(t, interp)[0], self.active_sh_degree,
                                     self.device, *self._maps, viewpoint_camera, pipe, bg_color, into, pixel_weight, scaling_modifier,
                                     cam_type, rgb8)

    render_contrib.__doc__ = _CONTRIB_DOC + """
        (There is no SparseBaked.select_rows: select on the dense bake, or prune the model, and bake sparse again.)"""

    def render_features(self, viewpoint_camera, pipe, bg_color, values, normalize=False, min_alpha=1e-4, scaling_modifier=1.0, cam_type=None,
                        interp="linear", rgb8=None, differentiable=False):
        return _render_features_state("SparseBaked.render_features", self, lambda t: self.state_at(t, interp)[0], self.active_sh_degree,
                                      self.device, *self._maps, viewpoint_camera, pipe, bg_color, values, normalize, min_alpha,
                                      scaling_modifier, cam_type, rgb8, differentiable)

    render_features.__doc__ = _FEATURES_DOC


def bake_sparse(pc, times, tol, max_bytes=None):
    """`bake` for a sequence in which much of the set hardly moves -> SparseBaked (its guarantees are listed there).

    tol: a float, or five in the order of FIELDS; absolute (world units for positions and scales, quaternion components, opacity, SH
    coefficients).  A negative value makes every row dynamic, math.inf keeps that field from deciding, NaN raises ValueError.
    Two passes over the timestamps, 2 * len(times) deformation forwards, so that the dense T x N storage never exists: the first puts the
    state at times[0] into the full working state and accumulates the extents (fdgs_state_extent), after which the list of dynamic rows is
    read back (the one synchronisation); the second deforms every timestamp again -- the forward is deterministic -- and keeps the dynamic
    rows (fdgs_state_gather).  Raises MemoryError, before allocating, when `max_bytes` is given and the full state alone exceeds it, and
    again when the full state and the compact rows do."""
    ts = _checked_times(times)
    tol = _checked_tol(tol)
    head_on, N = _checked_model(pc, "bake_sparse")
    T = len(ts)
    need = sparse_bake_bytes(N, 0, T, head_on)
    if max_bytes is not None and need > max_bytes:
        raise MemoryError(f"bake_sparse: the full state of {N} Gaussians needs {need} bytes, max_bytes = {max_bytes}")
    device = pc._xyz.device
    on = [h for h in range(len(FIELDS)) if head_on[h]]
    mask = _field_mask(head_on)
    with torch.no_grad():
        perm, forward = _deformer(pc)
        working = torch.empty(need // 4, dtype=torch.float32, device=device)          # (D = 0: the full state and nothing else)
        arrays = [v[0] for v in _carve(_field_slots(N), working)[1]]
        first, ext = _extent_pass(forward, ts, head_on, N, device)
        for dst, src in zip(arrays, first):
            dst.copy_(src)
        del first
        dyn = torch.zeros(N, dtype=torch.bool, device=device)
        for h in on:
            dyn |= ext[:, h] > tol[h]
        del ext
        found = torch.nonzero(dyn).reshape(-1).to(torch.int32)          # ascending; the one read-back
        D = int(found.shape[0])
        need = sparse_bake_bytes(N, D, T, head_on)
        if max_bytes is not None and need > max_bytes:
            raise MemoryError(f"bake_sparse: {D} dynamic rows of {N} at {T} timestamps need {need} bytes, max_bytes = {max_bytes}")
        storage = torch.empty(need // 4 - working.numel(), dtype=torch.float32, device=device)
        *per_field, (rows,) = _carve(_compact_slots(D, T, head_on), storage)[1]
        compact = [[v[k] if v else None for v in per_field] for k in range(T)]
        rows = rows.view(torch.int32)
        rows.copy_(found)
        if D and mask:
            for k, t in enumerate(ts):
                cur = forward(t)
                _lib.check(_lib.lib().fdgs_state_gather(_lib.stream_ptr(), D, _lib.ptr(rows), N, mask, _state_arrays(cur, mask),
                                                        _state_arrays(compact[k], mask)))
        if perm is not None:
            dyn = _deformation.permute_rows(perm, [dyn.to(torch.int32)], scatter=True)[0] != 0
    return SparseBaked(ts, head_on, perm, tol, working, arrays, storage, compact, rows, dyn, pc.active_sh_degree)


def pack_ply_rows(xyz, scales, rotations, opacity, shs):
    """The float32 [N,62] vertex table of io.write_ply_vertices from raw per-Gaussian arrays on the device (fdgs_pack_ply_rows):
    columns in the order of io.construct_list_of_attributes, SH coefficients channel-major as GaussianModel.save_ply stores them."""
    N = int(xyz.shape[0])
    c = lambda t, w: t.detach().float().contiguous().reshape(N, w)
    xyz, scales, rotations, opacity, shs = c(xyz, 3), c(scales, 3), c(rotations, 4), c(opacity, 1), c(shs, 48)
    if not _deformation._is_hip_device(xyz.device):
        raise _lib.FdgsError("pack_ply_rows runs on the GPU only")
    out = torch.empty(N, 62, dtype=torch.float32, device=xyz.device)
    _lib.check(_lib.lib().fdgs_pack_ply_rows(_lib.stream_ptr(), N, *[_lib.ptr(t) for t in (xyz, scales, rotations, opacity, shs, out)]))
    return out


def export_ply_sequence(pc, times, out_dir, pattern="time_{:05d}.ply"):
    """One static 3DGS point cloud per time, as export_perframe_3DGS.py writes them (gaussian_pertimestamp/time_00000.ply ...): the raw
    deformation outputs (deform(..., activate=False)) in GaussianModel.save_ply's format, rows in the model's order.  Per time: one
    deformation forward, one fdgs_pack_ply_rows launch, one device-to-host copy, one file.  Returns the paths."""
    if pc._features_dc.shape[1] != 1 or pc._features_rest.shape[1] != 15:
        raise ValueError("export_ply_sequence: SH degree 3 (16 coefficients), what the deformation's SH head produces")
    names = _io.construct_list_of_attributes(pc)
    paths = []
    with torch.no_grad():
        for k, t in enumerate(times):
            xyz, sc, rot, op, shs = _deformation.deform(pc._deformation, pc.get_xyz, pc._scaling, pc._rotation, pc._opacity,
                                                        shs_dc=pc._features_dc, shs_rest=pc._features_rest, time=float(t), activate=False)
            table = pack_ply_rows(xyz, sc, rot, op, shs).cpu().numpy()
            path = os.path.join(out_dir, pattern.format(k))
            _io.write_ply_vertices(path, names, table)
            paths.append(path)
    return paths
