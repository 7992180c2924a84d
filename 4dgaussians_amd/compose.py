"""Scene composition: several baked 4D models placed in one frame and rasterized once.

The reference's merge_many_4dgs.py deforms every model at the frame's time, moves each added model with a shift, a rotation and a scale,
concatenates all fields and rasterizes.  Here the models are `playback.Baked` states that stay in device memory, every model owns a fixed
range of rows of ONE composite state, and a frame is one fdgs_state_place launch per model whose time bracket changed -- the temporal
blend of the two bracketing baked frames fused into it -- followed by the rasterizer:

    scene = fdgs.compose.compose([baked_a, baked_b], [None, fdgs.compose.Placement(rotation=R, translation=d, scale=s)])
    for cam in cameras:
        out = scene.render(cam, pipe, background)               # the contract of Baked.render

A placement is a similarity transform (scale, then rotation, then shift -- the script's order).  mode="rigid" (the default) turns the
orientations of the splats and their view-dependent colour with the model: the placed model looks exactly like the model seen from the
inversely moved camera.  mode="points" is the script's own behaviour (`Placement.from_reference`): positions and scales only, so a turned
object keeps its splats and its highlights pointing the old way.  Fields of a model whose deformation head is off do not depend on the time
and are placed once, in `compose`.  No gradient flows through any of this.

With allow_sparse=True a model may also be a `playback.SparseBaked`: its whole working state is placed once, in `compose`, and a frame
places only its D dynamic rows, one fdgs_state_place_rows launch straight from the compact rows of the two bracketing timestamps:

    scene = fdgs.compose.compose([sparse_background, baked_actor], placements, allow_sparse=True)
"""
import math

import numpy as np
import torch

from . import _lib
from . import deformation as _deformation
from . import sh as _sh
from .playback import (_CONTRIB_DOC, _FEATURES_DOC, _MOTION_DOC, _PICK_DOC, BakedFrame, SparseBaked, _carve, _checked_interp, _field_mask,
                       _field_slots, _locate, _perm_maps, _render_contrib_state, _render_features_state, _render_motion_state, _render_pick_state,
                       _render_state, _state_arrays)

WRAPS = ("clamp", "loop", "pingpong")
_SH_ZERO = 1e-13        # entries of a band matrix below this are structural zeros of the rotation (the solve leaves ~1e-16 there)


def _fit_directions(n=64):
    """n well-spread unit directions (a Fibonacci spiral on the sphere), float64: the fixed sample sh_rotation fits on."""
    k = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
    r = np.sqrt(1.0 - z * z)
    return np.stack((r * np.cos(phi), r * np.sin(phi), z), axis=1)


def _basis64(dirs):
    """This package's SH basis (sh.basis, degree 3) at float64 directions [n,3] -> [n,16]."""
    return torch.cat(_sh.basis(3, torch.from_numpy(np.ascontiguousarray(dirs, dtype=np.float64))), dim=-1).numpy()


def sh_rotation(R):
    """(M1 [3,3], M2 [5,5], M3 [7,7]), float64: how the coefficients of SH bands 1 .. 3 mix when the model is turned by the rotation R.
    For every unit direction and coefficient row c [16]:  eval_sh(3, c @ blockdiag(1, M1, M2, M3), dir) == eval_sh(3, c, R^T dir),
    i.e. B(dir R) = B(dir) M^T for the basis row B.  Computed from sh.basis itself: the least-squares solution of B(D) X = B(D R) over 64
    fixed directions D (condition number 2.5), X = M^T; the off-block terms of X are rounding noise and only the diagonal blocks are kept.
    Entries below 1e-13 in magnitude are structural zeros and are returned as 0, so M(identity) is the identity exactly."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    D = _fit_directions()
    X = np.linalg.lstsq(_basis64(D), _basis64(D @ R), rcond=None)[0]
    out = []
    for l in (1, 2, 3):
        M = np.ascontiguousarray(X[l * l:(l + 1) ** 2, l * l:(l + 1) ** 2].T)
        M[np.abs(M) < _SH_ZERO] = 0.0
        out.append(M)
    return tuple(out)


def _quat_to_matrix(q):
    r, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                     [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                     [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]], dtype=np.float64)


def _matrix_to_quat(R):
    """Unit quaternion (r, x, y, z), r >= 0, of a rotation matrix (float64; the branch with the largest pivot)."""
    t = np.trace(R)
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        q = (0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s)
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = math.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = ((R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s)
    elif R[1, 1] > R[2, 2]:
        s = math.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = ((R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s)
    else:
        s = math.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = ((R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s)
    q = np.array(q, dtype=np.float64)
    q /= np.linalg.norm(q)
    return -q if q[0] < 0 else q


class Placement:
    """Where one model goes in the composite: x -> scale * x, turned by `rotation`, shifted by `translation`; and how its time runs.

    rotation: a 3x3 matrix (orthonormal, det +1, within 1e-6), a unit quaternion (r, x, y, z) (norm within 1e-6 of 1) or None (identity);
    scale: positive and finite; mode: "rigid" | "points" (see the module docstring); the model's frame time is
    map_time(times, t, placement) = wrap(time_scale * t + time_offset).  Anything else raises ValueError.

    The parameters are rounded to float32 ONCE, here; the object exposes what the kernel gets: `scale` (np.float32), `rotation` [3,3],
    `quat` [4], `translation` [3], `sh` = (M1, M2, M3) of sh_rotation(rotation given), all float32 numpy arrays."""

    def __init__(self, rotation=None, translation=(0.0, 0.0, 0.0), scale=1.0, mode="rigid", time_scale=1.0, time_offset=0.0, wrap="clamp"):
        if mode not in _lib.PLACE_MODES:
            raise ValueError(f"mode: 'rigid' or 'points', not {mode!r}")
        if wrap not in WRAPS:
            raise ValueError(f"wrap: one of {WRAPS}, not {wrap!r}")
        s = float(scale)
        if not (math.isfinite(s) and s > 0 and math.isfinite(float(np.float32(s))) and float(np.float32(s)) > 0):
            raise ValueError("scale: positive and finite")
        d = np.asarray(translation, dtype=np.float64).reshape(-1)
        if d.shape != (3,) or not np.isfinite(d).all():
            raise ValueError("translation: three finite numbers")
        if not (math.isfinite(float(time_scale)) and math.isfinite(float(time_offset))):
            raise ValueError("time_scale, time_offset: finite numbers")
        if rotation is None:
            R = np.eye(3)
        else:
            r = np.asarray(rotation.detach().cpu().numpy() if isinstance(rotation, torch.Tensor) else rotation, dtype=np.float64)
            if r.shape == (4,):
                if not np.isfinite(r).all() or abs(np.linalg.norm(r) - 1.0) > 1e-6:
                    raise ValueError("rotation: a UNIT quaternion (r, x, y, z)")
                R = _quat_to_matrix(r / np.linalg.norm(r))
            elif r.shape == (3, 3):
                if not np.isfinite(r).all() or np.abs(r @ r.T - np.eye(3)).max() > 1e-6 or abs(np.linalg.det(r) - 1.0) > 1e-6:
                    raise ValueError("rotation: an orthonormal 3x3 matrix with determinant +1")
                R = r
            else:
                raise ValueError("rotation: a 3x3 matrix, a unit quaternion (r, x, y, z) or None")
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        self.scale = np.float32(s)
        self.rotation, self.quat, self.translation = f32(R), f32(_matrix_to_quat(R)), f32(d)
        self.sh = tuple(f32(M) for M in sh_rotation(R))
        self.mode, self.wrap = mode, wrap
        self.time_scale, self.time_offset = float(time_scale), float(time_offset)

    @classmethod
    def from_reference(cls, motion_bias=(0.0, 0.0, 0.0), rotation_bias=(0.0, 0.0), scales_bias=1.0):
        """The arguments merge_many_4dgs.py takes for one added model: rotate_point_cloud(p, motion_bias, (theta, phi), scales_bias) =
        (p * scales_bias) @ (Rz(theta) Rx(phi))^T + motion_bias and scales * scales_bias, orientations and SH untouched (mode="points")."""
        theta, phi = (float(v) for v in rotation_bias)
        Rz = np.array([[math.cos(theta), -math.sin(theta), 0.0], [math.sin(theta), math.cos(theta), 0.0], [0.0, 0.0, 1.0]])
        Rx = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(phi), -math.sin(phi)], [0.0, math.sin(phi), math.cos(phi)]])
        return cls(rotation=Rz @ Rx, translation=[float(v) for v in motion_bias], scale=float(scales_bias), mode="points")

    def struct(self, sh_degree):
        """The fdgs_placement of this placement for a model of active SH degree `sh_degree`."""
        p = _lib.Placement()
        p.scale = float(self.scale)
        p.rot[:] = self.rotation.reshape(-1).tolist()
        p.quat[:] = self.quat.tolist()
        p.shift[:] = self.translation.tolist()
        p.sh1[:] = self.sh[0].reshape(-1).tolist()
        p.sh2[:] = self.sh[1].reshape(-1).tolist()
        p.sh3[:] = self.sh[2].reshape(-1).tolist()
        p.mode, p.sh_degree = _lib.PLACE_MODES[self.mode], int(sh_degree)
        return p


def map_time(times, t, placement):
    """The time a model with baked `times` is shown at when the composite's frame time is t (pure Python, float64):
    t' = placement.time_scale * t + placement.time_offset, wrapped onto [times[0], times[-1]].  A t' inside the range (both ends
    included) is returned as it is; outside, "clamp" takes the nearer end, "loop" repeats the range (t' modulo the span), "pingpong"
    runs it forwards and backwards.  A single timestamp maps to itself."""
    lo, hi = float(times[0]), float(times[-1])
    tp = placement.time_scale * float(t) + placement.time_offset
    span = hi - lo
    if span <= 0.0:
        return lo
    if lo <= tp <= hi:
        return tp
    if placement.wrap == "clamp" or not math.isfinite(tp):
        return lo if tp < lo else hi
    if placement.wrap == "loop":
        return lo + (tp - lo) % span
    x = (tp - lo) % (2.0 * span)
    return lo + (x if x <= span else 2.0 * span - x)


def compose_bytes(Ns):
    """Bytes `compose` stores for models of Ns[m] Gaussians: one placed state of sum(Ns) rows, each of its five arrays padded to
    playback.SLOT_ALIGN_FLOATS."""
    Ns = [int(n) for n in Ns]
    if not Ns or any(n < 0 for n in Ns):
        raise ValueError("compose_bytes: at least one model, N >= 0")
    return 4 * _carve(_field_slots(sum(Ns)))[0]


class Composite:
    """Several baked models in one world, as ONE placed state of sum(N) rows resident on the device.

    A SNAPSHOT like `Baked`: it refers to the baked frames of its models and holds placed copies.  Baking a model again, or changing a
    placement object afterwards, leaves it stale; compose again.

    A model that is a `SparseBaked` (compose(..., allow_sparse=True)) keeps that class's guarantees inside the composite, placed: compose()
    places all N rows of its working state once; a frame rewrites its D dynamic rows only (fdgs_state_place_rows), with the bits the dense
    composite holds for them; its static rows hold the placed state at times[0] for good.  With tol < 0 the composite is the composite of
    the dense bakes bit for bit; with tol = inf (D == 0) the model never launches.  The composite only READS its models: a SparseBaked's
    working state and its `launches` are not touched, and it keeps rendering on its own as before.

    `models`, `placements`, `N` (all rows), `offsets[m]` / `slices[m]` (model m's rows: [offset_m, offset_m + N_m), in that model's own row
    order for everything `render` returns), `nbytes` (== compose_bytes(Ns)), `active_sh_degree` (the maximum over the models; the bands a
    model does not have are stored as zeros), `launches` (fdgs_state_place and fdgs_state_place_rows launches so far, those of compose()
    included)."""

    def __init__(self, models, placements, storage, arrays):
        self.models, self.placements = tuple(models), tuple(placements)
        self._storage, self._arrays = storage, arrays
        self.N = int(arrays[0].shape[0])
        self.offsets, off = [], 0
        for m in self.models:
            self.offsets.append(off)
            off += m.N
        self.offsets = tuple(self.offsets)
        self.slices = tuple(slice(o, o + m.N) for o, m in zip(self.offsets, self.models))
        self.nbytes = storage.numel() * storage.element_size()
        self.active_sh_degree = max(m.active_sh_degree for m in self.models)
        self.launches = 0
        self._structs = [p.struct(m.active_sh_degree) for p, m in zip(self.placements, self.models)]
        self._shown = [None] * len(self.models)          # per model: the (i, j, w) its time-dependent rows hold
        self._frame = BakedFrame(arrays)
        self._masks = [_field_mask(m.head_on) for m in self.models]         # per model: its time-dependent fields
        self._maps = self._row_maps()
        self._targets = {}          # (m, mask) -> the fdgs_state_arrays of model m's rows: they never change, filled on first use
        self._motion_bufs = None
        self._pick_row_map = None

    @property
    def device(self):
        return self._storage.device

    def _target(self, m, mask):
        out = self._targets.get((m, mask))
        if out is None:
            out = self._targets[m, mask] = _state_arrays(self._arrays, mask, self.offsets[m])
        return out

    def _place(self, m, mask, i, j, w):
        model = self.models[m]
        if mask == 0 or model.N == 0:
            return
        blend = i != j
        if isinstance(model, SparseBaked):          # the D dynamic rows, from the compact rows of the two timestamps
            if model.D == 0:
                return
            _lib.check(_lib.lib().fdgs_state_place_rows(_lib.stream_ptr(), self._structs[m], model.D, _lib.ptr(model.rows), model.N, mask,
                                                        model._sources[i], model._sources[j] if blend else None,
                                                        float(w) if blend else 0.0, self._target(m, mask)))
        else:
            a, b = _state_arrays(model.frames[i].arrays(), mask), _state_arrays(model.frames[j].arrays(), mask)
            _lib.check(_lib.lib().fdgs_state_place(_lib.stream_ptr(), self._structs[m], model.N, mask, a, b if blend else None,
                                                   float(w) if blend else 0.0, self._target(m, mask)))
        self.launches += 1

    def _place_working_state(self, m):
        """All five fields of every row of a SparseBaked, from its working state: what its static rows and the fields whose head is off
        hold for good.  The dynamic rows hold whatever time the model showed last; the first frame overwrites them."""
        model = self.models[m]
        if model.N == 0:
            return
        mask = _field_mask([True] * len(model.head_on))
        _lib.check(_lib.lib().fdgs_state_place(_lib.stream_ptr(), self._structs[m], model.N, mask, _state_arrays(model._frame.arrays(), mask),
                                               None, 0.0, self._target(m, mask)))
        self.launches += 1

    def state_at(self, t, interp="linear"):
        """The composite state at frame time t as a BakedFrame over this object's arrays (overwritten by the next call): per model, ONE
        fdgs_state_place launch for its time-dependent fields, straight from the two baked frames that bracket map_time(times, t,
        placement) with the blend fused -- or no launch when that model's (i, j, w) is what its rows already hold.  A SparseBaked takes
        ONE fdgs_state_place_rows launch over its D dynamic rows instead, and none when D == 0."""
        _checked_interp(interp)
        for m, (model, pl, mask) in enumerate(zip(self.models, self.placements, self._masks)):
            if mask == 0:
                continue
            key = _locate(model.times, map_time(model.times, t, pl), interp)
            if key != self._shown[m]:
                self._place(m, mask, *key)
                self._shown[m] = key
        return self._frame

    def render(self, viewpoint_camera, pipe, bg_color, scaling_modifier=1.0, override_color=None, cam_type=None, interp="linear", rgb8=None):
        """The contract of `Baked.render` for the whole scene: the same raster settings (the PanopticSports dict camera included), the same
        result dict.  "radii" / "visibility_filter" have sum(N) entries, model m's at `slices[m]` in that model's own row order (segments
        of models stored through a permutation are scattered back); `override_color` is [sum(N), 3] in the same order."""
        return _render_state("Composite.render", lambda t: self.state_at(t, interp), self.active_sh_degree, self.device, *self._maps,
                             viewpoint_camera, pipe, bg_color, scaling_modifier, override_color, cam_type, rgb8)

    def render_motion(self, viewpoint_camera, pipe, bg_color, toward=None, toward_time=None, scaling_modifier=1.0, cam_type=None,
                      interp="linear", min_alpha=0.0, rgb8=None):
        return _render_motion_state("Composite.render_motion", self, lambda t: self.state_at(t, interp), self.active_sh_degree, self.device,
                                    *self._maps, viewpoint_camera, pipe, bg_color, toward, toward_time, scaling_modifier, cam_type, min_alpha,
                                    rgb8)

    render_motion.__doc__ = _MOTION_DOC + """
        Both times go through every model's own map_time; the motion of a placed model includes its placement."""

    def render_pick(self, viewpoint_camera, pipe, bg_color, scaling_modifier=1.0, cam_type=None, interp="linear", alpha_cut=0.5, rgb8=None):
        return _render_pick_state("Composite.render_pick", self, lambda t: self.state_at(t, interp), self.active_sh_degree, self.device,
                                  *self._maps, viewpoint_camera, pipe, bg_color, scaling_modifier, cam_type, alpha_cut, rgb8)

    render_pick.__doc__ = _PICK_DOC + """
        The ids are rows of the whole scene (sum(N), model m's at `slices[m]`): `model_of_rows` splits them into (model, row)."""

    def render_contrib(self, viewpoint_camera, pipe, bg_color, into=None, pixel_weight=None, scaling_modifier=1.0, cam_type=None,
                       interp="linear", rgb8=None):
        return _render_contrib_state("Composite.render_contrib", self, lambda t: self.state_at(t, interp), self.active_sh_degree, self.device,
                                     *self._maps, viewpoint_camera, pipe, bg_color, into, pixel_weight, scaling_modifier, cam_type, rgb8)

    render_contrib.__doc__ = _CONTRIB_DOC + """
        The rows are rows of the whole scene (sum(N), model m's at `slices[m]`; `model_of_rows` splits row indices into (model, row)).
        (There is no Composite.select_rows: select per model with `Baked.select_rows`, then compose again.)"""

    def render_features(self, viewpoint_camera, pipe, bg_color, values, normalize=False, min_alpha=1e-4, scaling_modifier=1.0, cam_type=None,
                        interp="linear", rgb8=None, differentiable=False):
        return _render_features_state("Composite.render_features", self, lambda t: self.state_at(t, interp), self.active_sh_degree, self.device,
                                      *self._maps, viewpoint_camera, pipe, bg_color, values, normalize, min_alpha, scaling_modifier, cam_type,
                                      rgb8, differentiable)

    render_features.__doc__ = _FEATURES_DOC + """
        The rows of `values` are rows of the whole scene (sum(N), model m's at `slices[m]`); with `model_indicator()` as the values the
        features are one matte per placed model, and they sum to "alpha"."""

    def model_indicator(self):
        """float32 [N, M] on the scene's device, M = len(models): row r holds a 1 in the column of the placed model that owns it (the row
        ranges `model_of_rows` splits ids by) and zeros elsewhere.  As the `values` of render_features: per-model mattes."""
        rows = torch.arange(sum(m.N for m in self.models), dtype=torch.int64, device=self.device)
        model = self.model_of_rows(rows)[0].to(torch.int64)
        out = torch.zeros(rows.shape[0], len(self.models), dtype=torch.float32, device=self.device)
        out[rows, model] = 1.0
        return out

    def _make_pick_row_map(self):
        """The stored -> scene row map of fdgs_render_pick: model m's segment is offset_m + perm_m (offset_m + arange for a model stored in
        its own order); None when no model is stored through a permutation."""
        if all(m.perm is None for m in self.models):
            return None
        segs = [(torch.arange(m.N, dtype=torch.int32, device=self.device) if m.perm is None else m.perm.to(torch.int32)) + o
                for m, o in zip(self.models, self.offsets)]
        return torch.cat(segs).to(torch.int32).contiguous()

    def model_of_rows(self, ids):
        """(model, row), int32 tensors of the shape of `ids` (rows of the scene, e.g. "pick_id" of render_pick): the index into `models`
        and the row inside that model, in its own order; both -1 where ids is -1."""
        ids = ids.to(torch.int64)
        starts = torch.tensor(self.offsets, dtype=torch.int64, device=ids.device)
        model = torch.bucketize(ids, starts, right=True) - 1          # the last model whose first row is <= id (empty models are skipped over)
        hit = ids >= 0
        model = torch.where(hit, model, torch.full_like(model, -1))
        row = torch.where(hit, ids - starts[model.clamp_min(0)], torch.full_like(ids, -1))
        return model.to(torch.int32), row.to(torch.int32)

    def _row_maps(self):
        """playback._perm_maps for the whole scene: model m's rows, `slices[m]`, go through model m's own permutation."""
        if all(m.perm is None for m in self.models):
            return None, None
        maps = [_perm_maps(m.perm) for m in self.models]

        def through(k):
            return lambda t: torch.cat([t[sl] if mp[k] is None else mp[k](t[sl]) for mp, sl in zip(maps, self.slices)])
        return through(0), through(1)


def compose(models, placements=None, max_bytes=None, allow_sparse=False):
    """Places `models` (a sequence of playback.Baked) in one world -> Composite.  placements[m] is a Placement or None (the identity);
    placements=None leaves every model where it is.  The composite owns ONE placed state of sum(N) rows: five arrays, each starting on a
    playback.SLOT_ALIGN_FLOATS boundary, model m in rows [offset_m, offset_m + N_m).  Fields whose head is off in a model do not depend on
    the time and are placed here, once; the others per frame (Composite.state_at).

    allow_sparse=True accepts any mix of Baked and playback.SparseBaked.  A sparse model's whole working state -- all five fields, all N
    rows -- is placed here, in one launch; a frame then places its D dynamic rows only (the guarantees are listed under `Composite`).  The
    opt-in is deliberate: such a composite inherits the tolerance band of its sparse models and is the dense composite bit for bit only
    where tol < 0.  compose_bytes and max_bytes are the same: the placed state has the same size.

    Raises TypeError for a model that is not a Baked (a playback.SparseBaked has no per-timestamp frames to place and needs
    allow_sparse=True), ValueError for models on different devices, MemoryError -- before anything is allocated -- when `max_bytes` is
    given and compose_bytes(...) exceeds it."""
    models = list(models)
    if not models:
        raise ValueError("compose: at least one model")
    if placements is None:
        placements = [None] * len(models)
    placements = [Placement() if p is None else p for p in placements]
    if len(placements) != len(models) or not all(isinstance(p, Placement) for p in placements):
        raise ValueError("compose: one Placement (or None) per model")
    for m in models:
        if isinstance(m, SparseBaked):
            if not allow_sparse:
                raise TypeError("compose: a model must be a playback.Baked (dense per-timestamp frames), not SparseBaked; "
                                "pass allow_sparse=True to place sparse bakes (the composite then inherits their tolerance band)")
        elif not hasattr(m, "frames"):
            raise TypeError(f"compose: a model must be a playback.Baked (dense per-timestamp frames), not {type(m).__name__}")
    device = models[0].device
    if any(m.device != device for m in models):
        raise ValueError("compose: every model must be on the same device")
    need = compose_bytes([m.N for m in models])
    if max_bytes is not None and need > max_bytes:
        raise MemoryError(f"compose: {sum(m.N for m in models)} Gaussians need {need} bytes, max_bytes = {max_bytes}")
    if not _deformation._is_hip_device(device):
        raise _lib.FdgsError("compose runs on the GPU only")
    total = sum(m.N for m in models)
    with torch.no_grad():
        storage = torch.empty(need // 4, dtype=torch.float32, device=device)
        arrays = [v[0] for v in _carve(_field_slots(total), storage)[1]]
        scene = Composite(models, placements, storage, arrays)
        for m, model in enumerate(models):
            if isinstance(model, SparseBaked):
                scene._place_working_state(m)
            else:
                scene._place(m, _field_mask([not on for on in model.head_on]), 0, 0, 0.0)
    return scene
