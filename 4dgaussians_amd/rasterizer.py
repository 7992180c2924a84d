"""Drop-in for the python package `diff_gaussian_rasterization` of the reference's rasterizer submodule.

Mirrors what the reference imports and calls at gaussian_renderer/__init__.py:14,38-58,120-128,
merge_many_4dgs.py:33,85-135 and scene/dataset_readers.py:485-508:

    GaussianRasterizationSettings(image_height, image_width, tanfovx, tanfovy, bg, scale_modifier, viewmatrix,
                                  projmatrix, sh_degree, campos, prefiltered, debug)      # plain picklable NamedTuple
    GaussianRasterizer(raster_settings)(means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None,
                                        rotations=None, cov3D_precomp=None) -> (color [3,H,W], radii [P] int32,
                                                                                depth [1,H,W])
    GaussianRasterizer(raster_settings, render_alpha=True)(...) -> (color, radii, depth, alpha [1,H,W])      # opt-in, differentiable
    GaussianRasterizer.markVisible(positions) -> bool [P]

All arithmetic runs in libfdgs.so (hand-written HIP for gfx950) through the C-ABI of include/fdgs.h; PyTorch only
supplies device memory, the current HIP stream and autograd bookkeeping.  There is no CPU fallback.
"""
import ctypes
import os
import threading
import warnings
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _lib
from ._lib import RasterGrads, RasterParams, check, ptr, stream_ptr


def _is_hip_device(dev):
    """(one predicate so that the host dry-run test can stand in for a device; there is no CPU path)"""
    return dev.type == "cuda"


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


class FrameOptions(NamedTuple):
    """What a frame asks of the rasterizer beyond colour, radii and depth; all off: the frame the reference renders.  `alpha`: the frame also
    delivers its accumulated opacity 1 - final_T.  `antialiasing`: the projection compensates every opacity for the 0.3 px dilation of its
    footprint.  `absgrad`: the frame's backward also returns the absolute screen-space gradients (include/fdgs.h at fdgs_raster_bwd_abs) and
    leaves them on the gradient sink of the screen-space means as its attribute `.absgrad`.  Built once per frame and handed on as itself;
    which C entry point each stage then calls: _stage_call."""
    alpha: bool = False
    antialiasing: bool = False
    absgrad: bool = False

    @classmethod
    def of(cls, source):
        """The options `source` asks for through its attributes `render_alpha`, `antialiasing` and `absgrad`: the `pipe` of render() (absent:
        off), a GaussianRasterizer."""
        return cls(bool(getattr(source, "render_alpha", False)), bool(getattr(source, "antialiasing", False)), bool(getattr(source, "absgrad", False)))

    def keywords(self):
        """rasterize_forward's keywords for what the frame asked.  A frame that asked for nothing passes none: its call is the one that
        function, and whatever a test puts in its place, has always received."""
        return {k: True for k, v in (("want_alpha", self.alpha), ("antialiasing", self.antialiasing), ("absgrad", self.absgrad)) if v}


PLAIN = FrameOptions()

# The suffixed forms each stage has beside its plain entry point (include/fdgs.h), and the one rule that picks among them:
#   antialiased -> the _aa form; it always takes the alpha image as its last argument, NULL where the frame did not ask for one;
#   alpha only  -> the _alpha form, with the image;
#   neither     -> the plain form, without the argument.
# The projection and the camera gradient have no alpha image, hence no _alpha form and no such argument; the blend has no _aa form: the
# projection carries the compensation, an antialiased frame blends like any other.
# The backward of a frame that asked for the absolute screen-space gradients has ONE form, fdgs_raster_bwd_abs, whatever else the frame asked:
# it takes the alpha gradient (or NULL), the antialiasing case as an int and the [P,3] output.
_STAGE_FORMS = {"preprocess_fwd": ("_aa",), "raster_fwd_capacity": ("_aa", "_alpha"), "render_fwd": ("_alpha",),
                "raster_bwd": ("_aa", "_alpha"), "camera_grad": ("_aa",)}


def _stage_call(L, stage, opts, args, alpha=None, absgrad=None):
    """fdgs_<stage> in the form `opts` selects, on `args`; `alpha`: the pointer of the alpha image (or of its gradient), for the forms that
    take one; `absgrad`: the pointer of the absolute screen-space gradients, for the backward of a frame that asked for them."""
    if stage == "raster_bwd" and opts.absgrad:
        check(L.fdgs_raster_bwd_abs(*args, alpha, 1 if opts.antialiasing else 0, absgrad))
        return
    forms = _STAGE_FORMS[stage]
    form = "_aa" if opts.antialiasing and "_aa" in forms else "_alpha" if opts.alpha and "_alpha" in forms else ""
    if form and "_alpha" in forms:
        args += (alpha,)
    check(getattr(L, "fdgs_" + stage + form)(*args))


# ---- pair-count bookkeeping of the binning stage -------------------------------------------------------------------------------------
# The reference's rasterizer reads the number of (tile, Gaussian) pairs back to the host in the middle of every forward (to size its
# binning buffer), with nothing queued behind the read: host and device wait for each other once per frame.  Here, once a pair count has
# been seen for (image size, number of Gaussians), the binning buffer is sized for a CAPACITY predicted from the largest count seen so far
# (x CAPACITY_SLACK) and the whole forward is queued by ONE C call (fdgs_raster_fwd_capacity).  BINNING selects what happens next:
#
#   "auto" (default)   VERIFIED: the host waits for the frame's pair count -- it reaches pinned host memory with the projection kernel, while
#                      the depth sort, the tile sort and the blending kernel are still queued, so the device does not drain -- and, if the
#                      count exceeds the capacity, finishes the frame EXACTLY (fdgs_bin_sort + fdgs_render_fwd on a buffer of the true size;
#                      stages 1-2 are complete in `geom`) before it returns.  No image that differs from the exact path ever leaves
#                      rasterize_forward (the reference never truncates a list: SURVEY Appendix B.2); `capacity_reruns` counts such frames.
#   "exact"            the reference's shape: four C calls, the blocking read-back between stage 2 and 3 (FDGS_BINNING=exact).  Also the
#                      first frame of every (size, count) pair in the other modes.
#   "capacity"         OPT-IN, never waits: the count is looked at when a later frame starts; a frame whose count exceeded its capacity has
#                      dropped pairs (binning form 1: its last tiles in image order, whole lists; form 0: its FARTHEST pairs) -- forward
#                      and backward alike, so its gradient is the exact gradient of the image it returned -- raises a RuntimeWarning and is counted in `capacity_overflows`.  For loops that prefer a host that runs
#                      a full frame ahead over the guarantee (the frame is then NOT the reference's).
# State is per host thread (threading.local): one thread drives a stream, as include/fdgs.h requires.
BINNING = os.environ.get("FDGS_BINNING", "auto")
CAPACITY_SLACK = 1.5
capacity_overflows = 0        # "capacity" mode: frames that dropped pairs
capacity_reruns = 0           # "auto" mode: frames finished exactly after their speculative capacity proved too small
_SENTINEL = 0xFFFFFFFF
_RING = 64
_tls = threading.local()
_seen = {}            # (device index, W, H, P) -> [largest pair count seen, P it was seen at]
_size_cache = {}      # ("geom", P) / ("img", W, H) / ("binning", R, W, H) -> bytes


class PairCount:
    """The pair count of one forward: known at once on the exact and verified paths, later in "capacity" mode (`value()` waits for it)."""
    __slots__ = ("addr", "capacity", "key", "P", "R", "stream", "buf")

    def poll(self):
        if self.R is None:
            v = ctypes.c_uint32.from_address(self.addr).value
            if v != _SENTINEL:
                self.R = v
                _note_count(self)
        return self.R

    def value(self):
        if self.poll() is None:
            self.stream.synchronize()
            self.poll()
        return self.R


def _note_count(c):
    global capacity_overflows
    e = _seen.get(c.key)
    if e is None:
        if len(_seen) > 64:
            _seen.clear()
        _seen[c.key] = [c.R, c.P]
    else:
        e[0] = max(e[0], c.R)
    if c.capacity is not None and c.R > c.capacity:
        capacity_overflows += 1
        warnings.warn(f"fdgs rasterizer (BINNING='capacity'): a frame listed {c.R} (tile, Gaussian) pairs but its binning buffer was sized for "
                      f"{c.capacity}: at least {c.R - c.capacity} pairs of that frame were dropped (its last tiles in image order; with binning "
                      "form 0 its farthest pairs); the capacity grows from the next frame on "
                      "(the default BINNING='auto' finishes such a frame exactly instead)", RuntimeWarning, stacklevel=3)


def _thread_state(dev):
    st = getattr(_tls, "st", None)
    if st is None:
        st = _tls.st = {"ring": {}, "pending": [], "last": None}
    ring = st["ring"].get(dev.index)
    if ring is None:
        ring = st["ring"][dev.index] = [_pinned_words(_RING), 0]
    return st, ring


def _pinned_words(n):
    return torch.zeros(n, dtype=torch.int32).pin_memory()


def _current_stream(dev):
    return torch.cuda.current_stream(dev)


def _bytes(L, kind, *args):
    key = (kind,) + args
    v = _size_cache.get(key)
    if v is None:
        nbytes = _lib.c_size_t()
        check(getattr(L, f"fdgs_{kind}_bytes")(*args, nbytes))
        if len(_size_cache) > 256:
            _size_cache.clear()
        v = _size_cache[key] = nbytes.value
    return v


def last_num_rendered():
    """Pair count of this thread's most recent forward (diagnostics; waits for the frame if its count has not arrived yet)."""
    st = getattr(_tls, "st", None)
    return 0 if st is None or st["last"] is None else int(st["last"].value())


def _f32(t, device):
    if t is None:
        return None
    if t.device != device:
        t = t.to(device)
    return (t if t.dtype == torch.float32 else t.float()).contiguous()


def _none_if_empty(t):
    return None if (t is None or t.numel() == 0) else t


class RasterState:
    """Buffers one forward pass leaves behind for its backward (the reference's geom/binning/img buffers).  `capacity` = the pair count
    the binning buffer is laid out for (what the C calls take as num_rendered); `num_rendered` = the true count (waits for it if needed)."""
    __slots__ = ("params", "geom", "binning", "img", "capacity", "count", "keep", "visibility", "acc", "with_alpha", "antialiasing", "absgrad")

    def take_accumulator(self):
        """(buffer, zeroed) for fdgs_raster_grads::scratch_acc: the [P,16] accumulator the forward zero-filled on the way (training frames), once;
        a second backward of the same state gets a fresh buffer that fdgs_raster_bwd fills itself."""
        acc, self.acc = self.acc, None
        if acc is not None:
            return acc, 1
        return torch.empty(self.params.P, 16, device=self.geom.device), 0

    @property
    def num_rendered(self):
        return int(self.count.value())

    @property
    def options(self):
        """The FrameOptions this frame was rendered with.  Read from the three slots on every call: the backward and the camera gradient
        follow the state as it is when they run."""
        return FrameOptions(self.with_alpha, self.antialiasing, self.absgrad)


def _check_inputs(shs, colors_precomp, scales, rotations, cov3D_precomp):
    """The reference's two input checks (its messages, typo included): one colour source, one covariance source."""
    if (shs is None) == (colors_precomp is None):
        raise Exception('Please provide excatly one of either SHs or precomputed colors!')
    if ((scales is None or rotations is None) and cov3D_precomp is None) or \
            ((scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')


def _frame_params(settings, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp):
    """(fdgs_raster_params of one frame, the eleven tensors it points at).  The tensors are normalised first: float32 and contiguous on the
    device of means3D, empty optional inputs -> None; visibility and acc_zero are rasterize_forward's to allocate."""
    dev = means3D.device
    means3D = _f32(means3D, dev)
    shs, colors_precomp = _f32(_none_if_empty(shs), dev), _f32(_none_if_empty(colors_precomp), dev)
    scales, rotations = _f32(_none_if_empty(scales), dev), _f32(_none_if_empty(rotations), dev)
    cov3D_precomp, opacities = _f32(_none_if_empty(cov3D_precomp), dev), _f32(opacities, dev)
    bg, view = _f32(settings.bg, dev), _f32(settings.viewmatrix, dev)
    proj, campos = _f32(settings.projmatrix, dev), _f32(settings.campos, dev)
    if means3D.shape[0] > 0:         # (an empty set may come without either)
        _check_inputs(shs, colors_precomp, scales, rotations, cov3D_precomp)
    P = means3D.shape[0]
    p = RasterParams()
    p.P, p.sh_degree, p.W, p.H = P, int(settings.sh_degree), int(settings.image_width), int(settings.image_height)
    p.sh_coeffs = 0 if shs is None else int(shs.numel() // max(P, 1) // 3)
    p.tanfovx, p.tanfovy, p.scale_modifier = float(settings.tanfovx), float(settings.tanfovy), float(settings.scale_modifier)
    p.prefiltered, p.debug = int(bool(settings.prefiltered)), int(bool(settings.debug))
    p.bg, p.viewmatrix, p.projmatrix, p.campos = ptr(bg), ptr(view), ptr(proj), ptr(campos)
    p.means3D, p.shs, p.colors_precomp, p.opacities = ptr(means3D), ptr(shs), ptr(colors_precomp), ptr(opacities)
    p.scales, p.rotations, p.cov3D_precomp = ptr(scales), ptr(rotations), ptr(cov3D_precomp)
    return p, (means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, bg, view, proj, campos)


def _claim_count(dev, key, P):
    """(the PairCount of a new forward: the next word of this thread's ring of pinned words, what the predictor has seen for `key`, the
    counts still in flight).  Counts of earlier frames that have arrived meanwhile feed the predictor on the way (never waits)."""
    tstate, ring = _thread_state(dev)
    pending = tstate["pending"]
    if pending:
        tstate["pending"] = pending = [c for c in pending if c.poll() is None]
    seen = _seen.get(key)
    cnt = PairCount()
    cnt.key, cnt.P, cnt.R, cnt.stream, cnt.capacity = key, P, None, None, None
    cnt.buf = ring[0]                    # (keeps the pinned ring alive for as long as anything may read or write this word)
    slot = ring[1] = (ring[1] + 1) % _RING
    cnt.addr = ring[0].data_ptr() + 4 * slot
    for c in pending:          # (a count still in flight in this slot -- 64 forwards old: cannot happen on a live device -- is waited for, never overwritten)
        if c.addr == cnt.addr:
            c.value()
    return cnt, seen, pending


def _finish_exact(L, st, p, geom, img, cnt, opts, color, depth, alpha):
    """Stages 3-4 on a binning buffer of the true size, cnt.R pairs (stages 1-2 are complete in `geom`) -> (binning, cnt.R).  A frame that
    asked for its accumulated opacity has the blend write that image, `alpha`, too."""
    binning = torch.empty(_bytes(L, "binning", cnt.R, p.W, p.H), dtype=torch.uint8, device=geom.device)
    check(L.fdgs_bin_sort(st, p, ptr(geom), ptr(binning), ptr(img), cnt.R))
    _stage_call(L, "render_fwd", opts, (st, p, ptr(geom), ptr(binning), ptr(img), cnt.R, ptr(color), ptr(depth)), ptr(alpha))
    return binning, cnt.R


def rasterize_forward(settings, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, out=None, expect_backward=False,
                      want_alpha=False, antialiasing=False, absgrad=False):
    """Runs stages 1-4 of include/fdgs.h. Returns (color, radii, depth, state).  `out` = (color [3,H,W], radii [P] int32, depth [1,H,W])
    buffers to write into (contiguous float32 / int32 on the device), e.g. slices of a batch tensor.  `expect_backward`: a training frame
    (the blending forward zero-fills the backward's accumulator on the way).  Which binning path runs: BINNING above -- every mode but the
    opt-in "capacity" returns the exact path's image.  `want_alpha` and `antialiasing` are the frame's FrameOptions: with `want_alpha` the
    result is (color, radii, depth, alpha [1,H,W], state), `out` has the alpha buffer as its fourth entry and the backward of `state` takes
    the alpha image's gradient (rasterize_backward's grad_alpha); with `antialiasing` every opacity is compensated (opacity * h,
    include/fdgs.h); with `absgrad` the forward is the one it would be without and the backward of `state` also returns the absolute
    screen-space gradients (rasterize_backward's means2D_abs).  All are recorded on `state`, whose backward and camera gradient follow it;
    which entry point each stage calls: _stage_call.  A frame that does not ask makes the C calls it always made."""
    global capacity_reruns
    opts = FrameOptions(bool(want_alpha), bool(antialiasing), bool(absgrad))
    L = _lib.lib()
    dev = means3D.device
    if not _is_hip_device(dev):
        raise _lib.FdgsError("the rasterizer runs on the GPU only (tensors must live on a HIP device)")
    p, tensors = _frame_params(settings, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp)
    P, W, H = p.P, p.W, p.H
    geom = torch.empty(_bytes(L, "geom", P), dtype=torch.uint8, device=dev)
    img = torch.empty(_bytes(L, "img", W, H), dtype=torch.uint8, device=dev)
    if out is None:
        out = (torch.empty(3, H, W, dtype=torch.float32, device=dev), torch.empty(P, dtype=torch.int32, device=dev),
               torch.empty(1, H, W, dtype=torch.float32, device=dev))
        if opts.alpha:
            out += (torch.empty(1, H, W, dtype=torch.float32, device=dev),)
    color, radii, depth = out[:3]
    alpha = out[3] if opts.alpha else None
    vis = torch.empty(P, dtype=torch.bool, device=dev)       # radii > 0, written by the projection kernel (no elementwise launch)
    p.visibility = ptr(vis)
    # a training frame: the blending forward zero-fills the backward's per-Gaussian accumulator on the way (no fill launch before the backward)
    acc = torch.empty(P, 16, device=dev) if expect_backward and P > 0 else None
    p.acc_zero = ptr(acc)
    st = stream_ptr()
    cnt, seen, pending = _claim_count(dev, (dev.index, W, H, P), P)      # (another model / a densified set: another key, i.e. one exact frame first)
    speculative = BINNING == "auto" or (BINNING == "capacity" and len(pending) < _RING - 2)
    if speculative and seen is not None and P > 0:
        cap = (int(seen[0] * CAPACITY_SLACK) + 8192) // 4096 * 4096
        ctypes.c_uint32.from_address(cnt.addr).value = _SENTINEL
        binning = torch.empty(_bytes(L, "binning", cap, W, H), dtype=torch.uint8, device=dev)
        _stage_call(L, "raster_fwd_capacity", opts, (st, p, ptr(geom), ptr(binning), ptr(img), cap, _lib.c_void_p(cnt.addr), ptr(radii), ptr(color),
                                                     ptr(depth)), ptr(alpha))
        if BINNING == "capacity":      # opt-in: never waits; the count is looked at when a later frame starts
            cnt.capacity = cap
            cnt.stream = _current_stream(dev)
            pending.append(cnt)
        else:                          # verified: the image this call returns is the exact path's
            true_n = _lib.c_uint32()
            check(L.fdgs_pair_count_wait(st, _lib.c_void_p(cnt.addr), true_n))
            cnt.R = true_n.value
            _note_count(cnt)
            if cnt.R > cap:            # the speculative frame dropped pairs: finish it exactly
                capacity_reruns += 1
                binning, cap = _finish_exact(L, st, p, geom, img, cnt, opts, color, depth, alpha)
    else:
        _stage_call(L, "preprocess_fwd", opts, (st, p, ptr(geom), ptr(radii)))
        check(L.fdgs_bin_prepare(st, p, ptr(geom), _lib.c_void_p(cnt.addr)))          # (blocks until the count is in host memory)
        cnt.R = ctypes.c_uint32.from_address(cnt.addr).value
        _note_count(cnt)
        binning, cap = _finish_exact(L, st, p, geom, img, cnt, opts, color, depth, alpha)
    _tls.st["last"] = cnt
    state = RasterState()
    state.params, state.geom, state.binning, state.img, state.capacity, state.count = p, geom, binning, img, cap, cnt
    state.visibility, state.acc, state.keep = vis, acc, tensors
    state.with_alpha, state.antialiasing, state.absgrad = opts
    if opts.alpha:
        return color, radii, depth, alpha, state
    return color, radii, depth, state


def fill_raster_grads(state, grad_color, grad_depth, d_means2D, epilogue=None):
    """The fdgs_raster_grads every backward of `state` starts from: the image gradients, where the screen-space gradient goes, the
    accumulator (state.take_accumulator: the one the forward zero-filled, once) and -- fused backward -- the deformation epilogue the
    per-Gaussian chain rule writes through instead of the other outputs.  Returns (g, accumulator); the caller keeps what g points at."""
    g = RasterGrads()
    acc, g.scratch_acc_zeroed = state.take_accumulator()
    g.dL_dcolor, g.dL_ddepth, g.dL_dmeans2D, g.scratch_acc = ptr(grad_color), ptr(grad_depth), ptr(d_means2D), ptr(acc)
    if epilogue is not None:
        g.deform_epilogue = ctypes.pointer(epilogue)
    return g, acc


def raster_bwd_call(L, state, g, grad_alpha=None, means2D_abs=None):
    """fdgs_raster_bwd of `state` on the filled fdgs_raster_grads `g`, in the form state.options selects (_stage_call).  `grad_alpha`
    [1,H,W] (contiguous float32): the gradient of the alpha image of a frame rendered with it, NULL where alpha did not reach the loss.
    `means2D_abs` [P,3] (contiguous float32): where an absgrad state's backward writes the absolute screen-space gradients; such a state
    must be given one (a NULL would silently be the call of a frame that did not ask)."""
    if state.absgrad and means2D_abs is None:
        raise _lib.FdgsError("the backward of a frame rendered with absgrad needs the means2D_abs buffer")
    _stage_call(L, "raster_bwd", state.options, (stream_ptr(), state.params, ptr(state.geom), ptr(state.binning), ptr(state.img), state.capacity, g),
                ptr(grad_alpha if state.with_alpha else None), ptr(means2D_abs if state.absgrad else None))


def camera_wants_grad(settings):
    """A frame asks for the camera's gradient when grad mode is on and viewmatrix, projmatrix or campos of its settings is a tensor that
    requires grad (a pose being refined, fdgs.camera.PoseDelta; tracking against a frozen model).  Read where the frame is built: inside
    autograd.Function.forward grad mode is always off."""
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                           for t in (settings.viewmatrix, settings.projmatrix, settings.campos))


def camera_gradients(state, acc):
    """fdgs_camera_grad behind fdgs_raster_bwd of `state`, on the accumulator `acc` that call used -> [48] floats: dL/dviewmatrix [0,16),
    dL/dprojmatrix [16,32), dL/dcampos [32,35) (include/fdgs.h).  Two launches, no atomics.  An antialiased state: the form of it that
    differentiates the compensation too (_stage_call)."""
    L = _lib.lib()
    p, dev = state.params, state.geom.device
    scratch = torch.empty(_bytes(L, "camera_grad_scratch", p.P), dtype=torch.uint8, device=dev)
    out = torch.empty(48, device=dev)
    _stage_call(L, "camera_grad", state.options, (stream_ptr(), p, ptr(state.geom), ptr(acc), ptr(scratch), ptr(out)))
    return out


def split_camera_gradients(out48, viewmatrix, projmatrix, campos):
    """The 48 floats of camera_gradients as gradients shaped (and typed, and placed) like the three camera tensors."""
    like = lambda g, t: None if not isinstance(t, torch.Tensor) else g.reshape(t.shape).to(device=t.device, dtype=t.dtype)
    return like(out48[:16], viewmatrix), like(out48[16:32], projmatrix), like(out48[32:35], campos)


def rasterize_backward(state, grad_color, grad_depth=None, camera=False, grad_alpha=None):
    """Backward of rasterize_forward. Returns dict of gradients (None where the input was absent).  `camera`: also the camera's gradient,
    as `viewmatrix` [4,4], `projmatrix` [4,4] and `campos` [3] (fdgs_camera_grad on the same accumulator, behind fdgs_raster_bwd).
    `grad_alpha`: the gradient of the alpha image of a frame rendered with want_alpha (None: it did not reach the loss).  A state rendered
    with absgrad also returns `means2D_abs` [P,3]: per Gaussian the sum over the pixels of the absolute screen-space gradient, in the units of
    `means2D`, third column 0 (include/fdgs.h at fdgs_raster_bwd_abs); any other state has no such key."""
    L = _lib.lib()
    p = state.params
    means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp = state.keep[:7]
    dev, P = means3D.device, p.P
    grad_color, grad_depth, grad_alpha = _f32(grad_color, dev), _f32(grad_depth, dev), _f32(grad_alpha, dev)
    if grad_alpha is not None and not state.with_alpha:
        raise _lib.FdgsError("grad_alpha for a frame that was rendered without alpha (rasterize_forward's want_alpha)")
    out = dict(means2D=torch.empty(P, 3, device=dev), means3D=torch.empty(P, 3, device=dev),
               opacities=torch.empty(P, 1, device=dev), colors=torch.empty(P, 3, device=dev),
               cov3D=torch.empty(P, 6, device=dev),
               shs=None if shs is None else torch.empty(P, p.sh_coeffs, 3, device=dev),
               scales=None if scales is None else torch.empty(P, 3, device=dev),
               rotations=None if rotations is None else torch.empty(P, 4, device=dev))
    g, scratch = fill_raster_grads(state, grad_color, grad_depth, out["means2D"])
    g.dL_dmeans3D, g.dL_dopacity, g.dL_dcolors, g.dL_dcov3D = ptr(out["means3D"]), ptr(out["opacities"]), ptr(out["colors"]), ptr(out["cov3D"])
    g.dL_dsh, g.dL_dscales, g.dL_drotations = ptr(out["shs"]), ptr(out["scales"]), ptr(out["rotations"])
    if state.absgrad:
        out["means2D_abs"] = torch.empty(P, 3, device=dev)
    raster_bwd_call(L, state, g, grad_alpha, out.get("means2D_abs"))
    if camera:
        c = out["camera"] = camera_gradients(state, scratch)       # (the call's 48 floats; the three below are views of it)
        out.update(viewmatrix=c[:16].reshape(4, 4), projmatrix=c[16:32].reshape(4, 4), campos=c[32:35])
    return out


# ---- the autograd nodes ---------------------------------------------------------------------------------------------------------------
# One forward and one backward body; each node class is the signature its frames record, around them.  Separate classes, so that a frame
# that does not ask for the camera's gradient records the node, with the inputs, it always recorded.

def leave_absgrad(sink, rows):
    """The contract of an absgrad frame (gsplat's means2d.absgrad): the tensor the caller passed as means2D -- render()'s
    result["viewspace_points"] -- gets the [P,3] float32 absolute screen-space gradients as its attribute `.absgrad`, ASSIGNED by every
    backward of the frame, never accumulated (a statistic of one backward, not a gradient)."""
    sink.absgrad = rows


def _node_forward(ctx, raster_settings, gaussians, expect_backward, opts, means2D=None):
    """`gaussians`: rasterize_forward's seven per-Gaussian inputs, in its order; `means2D`: the node's screen-space input."""
    _, sh, colors_precomp, opacities, scales, _, cov3Ds_precomp = gaussians
    *images, state = rasterize_forward(raster_settings, *gaussians, expect_backward=expect_backward, **opts.keywords())
    ctx.state = state
    ctx.absgrad_sink = means2D if opts.absgrad else None      # (the caller's tensor: its backward leaves .absgrad there; no cycle, it is an input)
    ctx.had = (sh is not None and sh.numel() > 0, colors_precomp is not None and colors_precomp.numel() > 0,
               scales is not None and scales.numel() > 0, cov3Ds_precomp is not None and cov3Ds_precomp.numel() > 0)
    ctx.shapes = (opacities.shape, None if sh is None else sh.shape)
    ctx.mark_non_differentiable(images[1])      # radii
    # an output the loss never used must arrive in backward as None, not as a materialised zero image: the
    # reference's training loss ignores `depth` (train.py:201-214), and a NULL dL_ddepth selects the blending
    # backward without the depth terms (render_bwd_kernel<false>, csrc/render.hip)
    ctx.set_materialize_grads(False)
    return tuple(images)        # (color, radii, depth) and, where asked for, alpha


def _node_backward(ctx, grad_color, grad_depth, grad_alpha, cam_at=None):
    """One gradient per input of the node: the eight Gaussian tensors come first; `cam_at`: where viewmatrix, projmatrix and campos sit
    (ctx.cam) in a node that has them as inputs.  A loss that saw depth or alpha but not the colour gets a zero colour image; rasterize_backward
    is given only the keywords the frame needs."""
    out = [None] * len(ctx.needs_input_grad)
    if grad_color is None:
        if grad_depth is None and grad_alpha is None:       # no image reached the loss
            return tuple(out)
        like = grad_depth if grad_depth is not None else grad_alpha
        grad_color = torch.zeros(3, ctx.state.params.H, ctx.state.params.W, device=like.device)
    kw = {} if cam_at is None else {"camera": True}
    if grad_alpha is not None:
        kw["grad_alpha"] = grad_alpha
    g = rasterize_backward(ctx.state, grad_color, grad_depth, **kw)
    if ctx.absgrad_sink is not None:
        leave_absgrad(ctx.absgrad_sink, g["means2D_abs"])
    had_sh, had_col, had_scale, had_cov = ctx.had
    op_shape, sh_shape = ctx.shapes
    out[:8] = (g["means3D"], g["means2D"], g["shs"].reshape(sh_shape) if had_sh else None, g["colors"] if had_col else None,
               g["opacities"].reshape(op_shape), g["scales"] if had_scale else None, g["rotations"] if had_scale else None,
               g["cov3D"] if had_cov else None)
    if cam_at is not None:
        out[cam_at:cam_at + 3] = split_camera_gradients(g["camera"], *ctx.cam)
    return tuple(out)


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, grad_mode=True,
                opts=PLAIN):
        return _node_forward(ctx, raster_settings, (means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp),
                             bool(grad_mode) and any(ctx.needs_input_grad), opts, means2D)

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth, grad_alpha=None):
        return _node_backward(ctx, grad_color, grad_depth, grad_alpha)


class _RasterizeGaussiansCamera(torch.autograd.Function):
    """The node of a frame whose camera asks for a gradient (camera_wants_grad): viewmatrix, projmatrix and campos of the settings are
    inputs as well, and their gradients come from fdgs_camera_grad behind the same fdgs_raster_bwd.  The Gaussians may all be detached
    (tracking)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrix, projmatrix, campos,
                raster_settings, opts=PLAIN):
        ctx.cam = (viewmatrix, projmatrix, campos)        # (shape / dtype / device of the gradients to return; inputs of this node anyway)
        return _node_forward(ctx, raster_settings, (means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp), True, opts,
                             means2D)

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth, grad_alpha=None):
        return _node_backward(ctx, grad_color, grad_depth, grad_alpha, cam_at=8)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, render_alpha=False,
                        antialiasing=False, absgrad=False):
    """-> (color, radii, depth), with `render_alpha` (color, radii, depth, alpha).  `antialiasing`: every opacity is compensated for the
    dilation of its footprint (rasterize_forward).  `absgrad`: every backward of the frame leaves the absolute screen-space gradients on
    `means2D` as `means2D.absgrad` (leave_absgrad)."""
    opts = FrameOptions(bool(render_alpha), bool(antialiasing), bool(absgrad))
    if camera_wants_grad(raster_settings):
        rs = raster_settings
        return _RasterizeGaussiansCamera.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                               rs.viewmatrix, rs.projmatrix, rs.campos, rs, opts)
    # (grad mode is read HERE: inside autograd.Function.forward it is always off and needs_input_grad stays True under torch.no_grad())
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                     raster_settings, torch.is_grad_enabled(), opts)


class GaussianRasterizer(nn.Module):
    # Opt-in opacity compensation of the 0.3 px dilation (upstream's `antialiasing`, gsplat's rasterize_mode="antialiased"): set it on the
    # instance, `rasterizer.antialiasing = True`.  An attribute, not a constructor argument: the constructor's parameter list is pinned
    # (tests/test_alpha_abi.py); rasterize_gaussians takes it as a keyword.
    antialiasing = False
    # Opt-in absolute screen-space gradients (AbsGS; gsplat's absgrad), set the same way: `rasterizer.absgrad = True`, then read
    # `means2D.absgrad` [P,3] of the tensor passed as means2D after a backward.
    absgrad = False

    def __init__(self, raster_settings, render_alpha=False):
        """`render_alpha`: forward also returns the accumulated opacity of every pixel, alpha [1,H,W] = 1 - final transmittance,
        differentiable like colour and depth -> (color, radii, depth, alpha)."""
        super().__init__()
        self.raster_settings = raster_settings
        self.render_alpha = bool(render_alpha)

    def markVisible(self, positions):
        L = _lib.lib()
        rs = self.raster_settings
        with torch.no_grad():
            pos = _f32(positions, positions.device)
            out = torch.empty(pos.shape[0], dtype=torch.uint8, device=pos.device)
            check(L.fdgs_mark_visible(stream_ptr(), pos.shape[0], ptr(pos), ptr(_f32(rs.viewmatrix, pos.device)),
                                      ptr(_f32(rs.projmatrix, pos.device)), ptr(out)))
        return out.bool()

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        _check_inputs(shs, colors_precomp, scales, rotations, cov3D_precomp)
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                   self.raster_settings, *FrameOptions.of(self))
