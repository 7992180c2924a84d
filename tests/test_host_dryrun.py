"""Host plumbing dry run (CPU, no kernels): fdgs.render / render_views forward + backward and the two-node path executed on CPU tensors
against a FAKE library object whose entry points only answer the size queries and the one read-back.  Nothing is computed -- the test
exists so that a Python-level slip (a missing slot, a wrong argument count, a None where a tensor is expected) is caught here and not on
the GPU box.  The product has no CPU path: the fake is installed by monkeypatch in this test only."""
import ctypes
import importlib

import pytest
import torch

fdgs = importlib.import_module("4dgaussians_amd")
syn = fdgs.synthetic


class _FakeLib:
    def __init__(self):
        self.calls = []
        self.record = False         # True: keep the non-pointer struct fields of the calls below (the front-end tests)
        self.deform, self.raster, self.epilogue = [], [], []
        self.pair_count = 7         # what the "device" counts for the next forward
        self.pairs, self.grads, self.bwd_views = [], [], []

    def __getattr__(self, name):
        if not name.startswith("fdgs_"):
            raise AttributeError(name)

        def fn(*a):
            self.calls.append(name)
            if self.record:
                self._note(name, a)
            if name in ("fdgs_geom_bytes", "fdgs_img_bytes", "fdgs_binning_bytes", "fdgs_deform_saved_bytes", "fdgs_deform_bwd_scratch_bytes"):
                a[-1].value = 4096
            elif name == "fdgs_bin_prepare":
                ctypes.cast(a[3], ctypes.POINTER(ctypes.c_uint32))[0] = self.pair_count
            elif name == "fdgs_raster_fwd_capacity":      # (the device would deliver the count later; the fake delivers it at once)
                ctypes.cast(a[6], ctypes.POINTER(ctypes.c_uint32))[0] = self.pair_count
            elif name == "fdgs_pair_count_wait":
                a[2].value = ctypes.cast(a[1], ctypes.POINTER(ctypes.c_uint32))[0]
            elif name == "fdgs_deform_bwd_live_tiles":
                for i in range(4):
                    a[3][i] = 1
            elif name == "fdgs_raster_bwd":
                g = a[6]
                self.acc_seen = getattr(self, "acc_seen", []) + [(int(g.scratch_acc or 0), int(g.scratch_acc_zeroed))]
            elif name == "fdgs_last_error":
                return b""
            elif name == "fdgs_abi_version":
                return 3
            return 0
        return fn

    def _note(self, name, a):
        if name == "fdgs_deform_fwd":
            p, out = a[1], a[2]
            self.deform.append(dict(N=p.N, C=p.C, L=p.L, W=p.W, head_on=list(p.head_on), activate=p.activate, shs_dc_stride=p.shs_dc_stride,
                                    shs_rest_stride=p.shs_rest_stride, time_scalar=p.time_scalar, saved_null=not out.saved,
                                    rot_norm_null=not out.rot_norm))
        elif name in ("fdgs_preprocess_fwd", "fdgs_raster_fwd_capacity"):
            p = a[1]
            self.raster.append({k: getattr(p, k) for k in ("P", "sh_degree", "sh_coeffs", "W", "H", "tanfovx", "tanfovy", "scale_modifier",
                                                           "prefiltered", "debug")})
            if name == "fdgs_raster_fwd_capacity":
                self.pairs.append(("raster_fwd_capacity", int(a[5])))       # (the capacity its binning buffer is laid out for)
        elif name in ("fdgs_bin_sort", "fdgs_render_fwd"):
            self.pairs.append((name[len("fdgs_"):], int(a[5])))       # (the pair count the binning buffer is laid out for)
        elif name == "fdgs_deform_bwd":       # whose activated outputs / rotation norms this deformation backward reads
            self.bwd_views.append((a[2].out_scales, a[2].out_rotations, a[2].out_opacity, a[2].rot_norm))
        elif name == "fdgs_raster_bwd":
            g = a[6]
            self.grads.append(" ".join(k for k, _ in g._fields_ if getattr(g, k)))      # the non-NULL pointers (and scratch_acc_zeroed = 1)
            if g.deform_epilogue:
                e = g.deform_epilogue.contents
                self.epilogue.append((e.assign, e.tile_flags, e.activate, e.Npad, e.zero_floats))


@pytest.fixture
def fake(monkeypatch):
    f = _FakeLib()
    monkeypatch.setattr(fdgs._lib, "lib", lambda: f)
    monkeypatch.setattr(fdgs._lib, "stream_ptr", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(fdgs.rasterizer, "stream_ptr", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(fdgs.deformation, "stream_ptr", lambda: ctypes.c_void_p(0), raising=False)
    monkeypatch.setattr(fdgs.rasterizer, "_pinned_words", lambda n: torch.zeros(n, dtype=torch.int32))
    monkeypatch.setattr(fdgs.rasterizer, "_current_stream", lambda dev: type("S", (), {"synchronize": lambda self: None})())
    monkeypatch.setattr(fdgs.rasterizer, "_tls", __import__("threading").local())
    monkeypatch.setattr(fdgs.rasterizer, "_seen", {})
    monkeypatch.setattr(fdgs.rasterizer, "_size_cache", {})
    # rasterize_forward / forward_impl refuse non-HIP tensors: the dry run claims to be one
    monkeypatch.setattr(fdgs.rasterizer, "_is_hip_device", lambda dev: True)
    monkeypatch.setattr(fdgs.deformation, "_is_hip_device", lambda dev: True)
    return f


class _Pipe:
    convert_SHs_python = False
    compute_cov3D_python = False
    debug = False


@pytest.mark.parametrize("fused", [True, False])
def test_render_forward_backward_plumbing(fake, fused, monkeypatch):
    monkeypatch.setattr(fdgs.renderer, "FUSED_BACKWARD", fused)
    pc = syn.SynthModel(300, "dynerf_default", seed=1)
    cam = syn.make_camera(64, 48, theta_deg=10.0, time=0.3)
    res = fdgs.render(cam, pc, _Pipe(), torch.zeros(3), stage="fine")
    assert set(res) == {"render", "viewspace_points", "visibility_filter", "radii", "depth"}
    assert res["visibility_filter"].dtype == torch.bool and res["visibility_filter"].shape == (300,)
    res["render"].sum().backward()
    assert pc._xyz.grad is not None and res["viewspace_points"].grad is not None
    assert "fdgs_raster_bwd" in fake.calls and "fdgs_deform_bwd" in fake.calls
    # coarse stage and a no-grad forward
    with torch.no_grad():
        fdgs.render(cam, pc, _Pipe(), torch.zeros(3), stage="coarse")


def test_backward_accumulator_is_the_one_the_forward_zero_filled_exactly_once(fake):
    """A training frame allocates the blending backward's [P,16] accumulator at forward time and has fdgs_render_fwd zero-fill it on the way
    (fdgs_raster_params::acc_zero): the first backward of that state hands it over with scratch_acc_zeroed = 1 (no fill launch), a second
    backward of the same graph gets a fresh buffer that fdgs_raster_bwd must fill itself; a no-grad frame allocates none."""
    R = fdgs.rasterizer
    pc = syn.SynthModel(300, "dynerf_default", seed=1)
    cam = syn.make_camera(64, 48, theta_deg=10.0, time=0.3)
    res = fdgs.render(cam, pc, _Pipe(), torch.zeros(3), stage="fine")
    res["render"].sum().backward(retain_graph=True)
    res["render"].sum().backward()
    (a0, z0), (a1, z1) = fake.acc_seen
    assert a0 != 0 and a1 != 0 and z0 == 1 and z1 == 0
    st = R.RasterState()
    st.acc, st.params, st.geom = None, type("P", (), {"P": 5})(), torch.zeros(1)
    buf, zeroed = st.take_accumulator()
    assert buf.shape == (5, 16) and zeroed == 0
    with torch.no_grad():
        fdgs.render(cam, pc, _Pipe(), torch.zeros(3), stage="fine")
    assert len(fake.acc_seen) == 2


def test_render_views_plumbing(fake):
    pc = syn.SynthModel(200, "dnerf_bouncingballs", seed=2)
    cams = [syn.make_camera(64, 48, theta_deg=10.0 * i, time=0.1 * i) for i in range(3)]
    res = fdgs.render_views(cams, pc, _Pipe(), torch.zeros(3), stage="fine")
    assert len(res) == 3
    sum(r["render"].sum() for r in res).backward()
    assert all(r["viewspace_points"].grad is not None for r in res) and pc._xyz.grad is not None


def test_gradient_arena_layout_tiles_the_arena_without_overlap():
    """deformation._arena_layout: every view starts 256-byte aligned, views do not overlap, the planes' strides are channels-last and the
    per-Gaussian head ends where the zero-filled part begins; _collect caches per module and notices a replaced parameter."""
    d = fdgs.deformation
    planes = ((1, 16, 64, 64), (1, 16, 25, 64), (1, 16, 64, 25))
    mlps = ((128, 32), (128,), (3, 128), (3,))
    for combined in (True, False):
        total, head, n_fixed, specs = d._arena_layout(1000, combined, planes, mlps)
        assert n_fixed == (5 if combined else 6) and len(specs) == n_fixed + len(planes) + len(mlps)
        arena = torch.zeros(total)
        spans = []
        for i, (shape, strides, off) in enumerate(specs):
            assert off % 64 == 0
            v = arena.as_strided(shape, strides, off)
            n = v.numel()
            spans.append((off, off + n))
            v.fill_(float(i + 1))
            if n_fixed <= i < n_fixed + len(planes):
                assert v.is_contiguous(memory_format=torch.channels_last) and tuple(v.shape) == planes[i - n_fixed]
            else:
                assert v.is_contiguous()
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= total
        assert head == specs[n_fixed][2]
        for i, (shape, strides, off) in enumerate(specs):      # nobody wrote into anybody else's slice
            assert bool((arena.as_strided(shape, strides, off) == float(i + 1)).all())
    net = syn.SynthModel(50, "dynerf_default", seed=3)._deformation
    a = d._collect(net)
    b = d._collect(net)
    assert a[0] is b[0] and a[1] is b[1]
    seq = getattr(net.deformation_net, d.HEAD_NAMES[-1])
    seq[3].bias = torch.nn.Parameter(seq[3].bias.detach().clone())
    c = d._collect(net)
    assert c[1] is not a[1] and c[1][-1] is seq[3].bias
    # an INTERIOR parameter, a whole head and a grid level replaced: each is noticed (every cached slot is re-validated on every call)
    dn = net.deformation_net
    lin = getattr(dn, d.HEAD_NAMES[1])[1]
    lin.weight = torch.nn.Parameter(lin.weight.detach().clone())
    e = d._collect(net)
    assert e[1] is not c[1] and any(t is lin.weight for t in e[1])
    import copy
    setattr(dn, d.HEAD_NAMES[2], copy.deepcopy(getattr(dn, d.HEAD_NAMES[2])))
    f = d._collect(net)
    assert f[1] is not e[1] and any(t is getattr(dn, d.HEAD_NAMES[2])[3].weight for t in f[1])
    dn.grid.grids[0] = copy.deepcopy(dn.grid.grids[0])
    g = d._collect(net)
    assert g[0] is not f[0] and g[0][0] is dn.grid.grids[0][0]
    assert d._collect(net)[0] is g[0]                      # ... and an untouched module hits the cache
    # the cache lives on the module: nothing global keeps a deleted model's Parameters alive
    import gc
    import weakref
    w = weakref.ref(net.deformation_net.grid.grids[0][0])
    del net, a, b, c, e, f, g, dn, lin, seq
    gc.collect()
    assert w() is None


def test_host_time_per_frame_stays_within_budget(fake):
    """Python / ctypes / autograd time of one render() forward + backward against the fake library (no kernels, no device): what the host must
    spend per frame before any launch cost.  Measured 0.78 ms on the build container (0.15 ms forward only, where render() calls the two stages
    directly instead of through autograd.Function.apply; ~0.3 ms of the 0.78 is the autograd engine
    handing 46 gradients to their AccumulateGrad nodes): a frame whose GPU work is shorter than this is host-paced (BASELINE config 2 sits at
    0.8 ms of GPU work).  The budget is 2x the measurement -- loose enough for a loaded CI host, tight enough to catch a per-frame module walk,
    a per-tensor conversion pass or a re-introduced host synchronisation."""
    import time
    fake.calls = type("Sink", (), {"append": lambda self, x: None})()
    pc = syn.SynthModel(300, "dynerf_default", seed=1)
    cam = syn.make_camera(64, 48, theta_deg=10.0, time=0.3)
    bg, dimg = torch.zeros(3), torch.ones(3, 48, 64)
    prm = [p for p in pc.parameters() if p.requires_grad]

    def step():
        for p in prm:
            p.grad = None
        fdgs.render(cam, pc, _Pipe(), bg, stage="fine")["render"].backward(dimg)

    for _ in range(30):
        step()
    best = float("inf")
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(100):
            step()
        best = min(best, (time.perf_counter() - t0) / 100 * 1e3)
    print(f"host time per render() forward + backward: {best:.3f} ms")
    assert best < 1.7, best


# ---- the frame front end: what render, render_views, playback and compose hand to the library ---------------------------------------------
# Every literal below was recorded at the commit BEFORE render / render_views / bake / Baked.render / Composite.render came to share one
# camera block, one deformation plan, one render body and one slot layout: they pin that commit's behaviour.  N = 300 takes the models'
# own row order, N = 8200 (>= renderer.IMPLICIT_ORDER_MIN_N, a random cube) the implicit Hilbert permutation.

P, C = fdgs.playback, fdgs.compose
TIMES = (0.0, 0.5, 1.0)
SIZES = (300, 8200)


def _model(n, cfg="dynerf_default", seed=1):
    return syn.SynthModel(n, cfg, seed=seed)


def _cam(t=0.5, theta=10.0):
    return syn.make_camera(64, 48, theta_deg=theta, time=t)


def _colors(n):
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(4))


def _run_bake(fake, n):
    pc = _model(n)
    fake.calls.clear()
    P.bake(pc, TIMES)


def _run_baked_render(fake, n):
    baked = P.bake(_model(n), TIMES)
    fake.calls.clear()
    out = baked.render(_cam(0.5), _Pipe(), torch.zeros(3), rgb8="trunc")
    assert out["rgb8"].shape == (48, 64, 3) and out["viewspace_points"] is None
    fake.calls.append("fdgs_--")
    out = baked.render(_cam(0.25), _Pipe(), torch.zeros(3), override_color=_colors(n))
    assert out["radii"].shape == (n,) and out["visibility_filter"].dtype == torch.bool


def _run_bake_sparse(fake, n):
    pc = _model(n)
    fake.calls.clear()
    sb = P.bake_sparse(pc, TIMES, tol=-1.0)
    assert sb.D == n and sb.nbytes == P.sparse_bake_bytes(n, n, len(TIMES), sb.head_on)


def _run_sparse_render(fake, n):
    sb = P.bake_sparse(_model(n), TIMES, tol=-1.0)
    fake.calls.clear()
    sb.render(_cam(0.5), _Pipe(), torch.zeros(3), rgb8="round")
    fake.calls.append("fdgs_--")
    out = sb.render(_cam(0.25), _Pipe(), torch.zeros(3), override_color=_colors(n))
    assert out["radii"].shape == (n,) and sb.launches == 2


def _run_motion_extent(fake, n):
    pc = _model(n)
    fake.calls.clear()
    assert P.motion_extent(pc, TIMES).shape == (n, 5)


def _two_baked(n):
    return [P.bake(_model(n, seed=1), TIMES), P.bake(_model(n, "dnerf_bouncingballs", seed=2), TIMES)]


def _run_compose(fake, n):
    models = _two_baked(n)
    fake.calls.clear()
    scene = C.compose(models, [None, C.Placement(rotation=(0.0, 1.0, 0.0, 0.0), translation=(0.5, 0.0, -0.25), scale=0.5)])
    assert scene.N == 2 * n and scene.nbytes == C.compose_bytes([n, n])


def _run_composite_render(fake, n):
    scene = C.compose(_two_baked(n), [None, C.Placement(translation=(0.5, 0.0, -0.25), scale=0.5, time_offset=0.1)])
    fake.calls.clear()
    scene.render(_cam(0.5), _Pipe(), torch.zeros(3), rgb8="trunc")
    fake.calls.append("fdgs_--")
    out = scene.render(_cam(0.25), _Pipe(), torch.zeros(3), override_color=_colors(2 * n))
    assert out["radii"].shape == (2 * n,) and out["viewspace_points"] is None


def _run_render_nograd(fake, n):
    pc = _model(n)
    fake.calls.clear()
    with torch.no_grad():
        fdgs.render(_cam(0.5), pc, _Pipe(), torch.zeros(3), stage="fine")
        fake.calls.append("fdgs_--")
        fdgs.render(_cam(0.25), pc, _Pipe(), torch.zeros(3), stage="fine")


def _run_render_backward(fake, n):
    pc = _model(n)
    fake.calls.clear()
    res = fdgs.render(_cam(0.5), pc, _Pipe(), torch.zeros(3), stage="fine")
    res["render"].sum().backward()
    assert pc._xyz.grad.shape == (n, 3) and res["viewspace_points"].grad.shape == (n, 3)


def _run_render_views(fake, n):
    pc = _model(n, "dnerf_bouncingballs", seed=2)
    fake.calls.clear()
    res = fdgs.render_views([_cam(0.1 * i, 10.0 * i) for i in range(3)], pc, _Pipe(), torch.zeros(3), stage="fine")
    sum(r["render"].sum() for r in res).backward()
    assert all(r["viewspace_points"].grad.shape == (n, 3) and r["radii"].shape == (n,) for r in res)


_RUNS = dict(bake=_run_bake, baked_render=_run_baked_render, bake_sparse=_run_bake_sparse, sparse_render=_run_sparse_render,
             motion_extent=_run_motion_extent, compose=_run_compose, composite_render=_run_composite_render,
             render_nograd=_run_render_nograd, render_backward=_run_render_backward, render_views=_run_render_views)


def _calls_of(fake, entry, n):
    """The ordered fdgs_* calls of one entry point, prefix dropped; "--" separates two calls of it."""
    _RUNS[entry](fake, n)
    return " ".join(c[len("fdgs_"):] for c in fake.calls)


_FWD = "deform_pack_bytes deform_fwd"
_EXACT = "geom_bytes img_bytes preprocess_fwd bin_prepare binning_bytes bin_sort render_fwd"
_CAP = "binning_bytes raster_fwd_capacity pair_count_wait"
_BWD = "tuning_get raster_bwd deform_bwd"
PARENT_CALLS = {
    ('bake', 300): f"{_FWD} {_FWD} {_FWD}",
    ('bake', 8200): f"permute_rows {_FWD} {_FWD} {_FWD}",
    ('bake_sparse', 300): f"{_FWD} {_FWD} state_extent {_FWD} state_extent {_FWD} state_gather {_FWD} state_gather {_FWD} state_gather",
    ('bake_sparse', 8200): f"permute_rows {_FWD} {_FWD} state_extent {_FWD} state_extent {_FWD} state_gather {_FWD} state_gather {_FWD} state_gather permute_rows",
    ('baked_render', 300): f"{_EXACT} image_rgb8 -- state_blend {_CAP}",
    ('baked_render', 8200): f"{_EXACT} permute_rows image_rgb8 -- state_blend permute_rows {_CAP} permute_rows",
    ('compose', 300): f"state_place",
    ('compose', 8200): f"state_place",
    ('composite_render', 300): f"state_place state_place {_EXACT} image_rgb8 -- state_place state_place {_CAP}",
    ('composite_render', 8200): f"state_place state_place {_EXACT} permute_rows permute_rows image_rgb8 -- state_place state_place permute_rows permute_rows {_CAP} permute_rows permute_rows",
    ('motion_extent', 300): f"{_FWD} {_FWD} state_extent {_FWD} state_extent",
    ('motion_extent', 8200): f"permute_rows {_FWD} {_FWD} state_extent {_FWD} state_extent permute_rows",
    ('render_backward', 300): f"deform_saved_bytes {_FWD} {_EXACT} deform_bwd_scratch_bytes {_BWD}",
    ('render_backward', 8200): f"permute_rows deform_saved_bytes {_FWD} {_EXACT} permute_rows deform_bwd_scratch_bytes {_BWD} permute_rows",
    ('render_nograd', 300): f"{_FWD} {_EXACT} -- {_FWD} {_CAP}",
    ('render_nograd', 8200): f"permute_rows {_FWD} {_EXACT} permute_rows -- permute_rows {_FWD} {_CAP} permute_rows",
    ('render_views', 300): f"deform_saved_bytes {_FWD} {_EXACT} deform_saved_bytes {_FWD} {_CAP} deform_saved_bytes {_FWD} raster_fwd_capacity pair_count_wait deform_bwd_scratch_bytes {_BWD} {_BWD} {_BWD}",
    ('render_views', 8200): f"permute_rows permute_rows deform_saved_bytes {_FWD} {_EXACT} deform_saved_bytes {_FWD} {_CAP} deform_saved_bytes {_FWD} raster_fwd_capacity pair_count_wait permute_rows deform_bwd_scratch_bytes {_BWD} {_BWD} {_BWD} permute_rows permute_rows",
    ('sparse_render', 300): f"state_scatter {_EXACT} image_rgb8 -- state_scatter {_CAP}",
    ('sparse_render', 8200): f"state_scatter {_EXACT} permute_rows image_rgb8 -- state_scatter permute_rows {_CAP} permute_rows",
}


PARENT_DEFORM_RECORD = {"N": 300, "C": 16, "L": 2, "W": 128, "head_on": [1, 1, 1, 1, 1], "activate": 1, "shs_dc_stride": 3, "shs_rest_stride": 45, "time_scalar": 0.5, "saved_null": True, "rot_norm_null": False}
PARENT_RASTER_RECORD = {
    False: {"P": 300, "sh_degree": 3, "sh_coeffs": 16, "W": 64, "H": 48, "tanfovx": 0.36000001430511475, "tanfovy": 0.27000001072883606, "scale_modifier": 0.75, "prefiltered": 0, "debug": 0},
    True: {"P": 300, "sh_degree": 2, "sh_coeffs": 16, "W": 56, "H": 40, "tanfovx": 0.44999998807907104, "tanfovy": 0.30000001192092896, "scale_modifier": 0.75, "prefiltered": 0, "debug": 1},
}
PARENT_EPILOGUE_RENDER = [(1, 1, 1, 384, 2460096)]
PARENT_EPILOGUE_VIEWS = [(1, 1, 1, 384, 0), (0, 1, 1, 384, 0), (0, 1, 1, 384, 0)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("entry", sorted(_RUNS))
def test_entry_points_make_the_calls_they_made_before_the_front_end_was_shared(fake, entry, n):
    assert _calls_of(fake, entry, n) == PARENT_CALLS[entry, n]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cfg", ["dynerf_default", "dnerf_bouncingballs", "hypernerf_default"])
def test_bake_bake_sparse_and_motion_extent_deform_exactly_as_render_does_without_grad(fake, cfg, n):
    """The bit-equality of baked playback with fdgs.render under torch.no_grad() rests on this: at one time value every entry point fills
    the same fdgs_deform_params and asks for neither saved activations nor (activate being on) a missing rot_norm."""
    fake.record = True
    pc = _model(n, cfg, seed=3)

    def records(run):
        fake.deform.clear()
        run()
        return list(fake.deform)

    def live():
        with torch.no_grad():
            for t in TIMES:
                fdgs.render(_cam(t), pc, _Pipe(), torch.zeros(3), stage="fine")

    want = records(live)
    assert [r["time_scalar"] for r in want] == list(TIMES) and all(r["N"] == n and r["saved_null"] and not r["rot_norm_null"] for r in want)
    assert records(lambda: P.bake(pc, TIMES)) == want
    assert records(lambda: P.motion_extent(pc, TIMES)) == want
    assert records(lambda: P.bake_sparse(pc, TIMES, tol=-1.0)) == want + want          # the extent pass, then the gather pass
    if cfg == "dynerf_default":
        assert want[1] == PARENT_DEFORM_RECORD | {"N": n}


@pytest.mark.parametrize("panoptic", [False, True])
def test_render_baked_render_and_composite_render_hand_the_rasterizer_the_same_settings(fake, panoptic):
    fake.record = True
    pc = _model(300)
    bg, pipe = torch.tensor([0.1, 0.2, 0.3]), _Pipe()
    cam, kw = _cam(0.5), {}
    if panoptic:
        settings = fdgs.rasterizer.GaussianRasterizationSettings(
            image_height=40, image_width=56, tanfovx=0.45, tanfovy=0.3, bg=bg, scale_modifier=0.75, viewmatrix=cam.world_view_transform,
            projmatrix=cam.full_proj_transform, sh_degree=2, campos=cam.camera_center, prefiltered=False, debug=True)
        cam, kw = {"camera": settings, "time": 0.5}, {"cam_type": "PanopticSports"}
    with torch.no_grad():
        fdgs.render(cam, pc, pipe, bg, 0.75, stage="fine", **kw)
    baked = P.bake(pc, TIMES)
    baked.render(cam, pipe, bg, 0.75, **kw)
    C.compose([baked]).render(cam, pipe, bg, 0.75, **kw)
    live, from_baked, from_scene = fake.raster
    assert live == from_baked == from_scene == PARENT_RASTER_RECORD[panoptic]
    assert fake.deform[0]["time_scalar"] == 0.5


def test_fused_backwards_fill_the_epilogue_as_before(fake):
    """(assign, tile_flags, activate, Npad, zero_floats) of fdgs_raster_deform_epilogue: the single-view backward assigns and has the kernel
    clear the rest of the arena; of three views behind one node only the first processed one assigns, and none clears."""
    fake.record = True
    _run_render_backward(fake, 300)
    assert fake.epilogue == PARENT_EPILOGUE_RENDER
    fake.epilogue.clear()
    _run_render_views(fake, 300)
    assert fake.epilogue == PARENT_EPILOGUE_VIEWS and [e[0] for e in fake.epilogue] == [1, 0, 0]


# ---- the rasterizer's host side: recorded at the commit BEFORE its stage arguments and the fused backward body came to be written once -------
PARENT_RERUN_CALLS = f"{_CAP} binning_bytes bin_sort render_fwd"
PARENT_RERUN_PAIRS = [("raster_fwd_capacity", 8192), ("bin_sort", 9426), ("render_fwd", 9426)]
PARENT_RERUN_STATE = (1, 0, 9426, 9426, 9426)        # capacity_reruns gained, capacity_overflows, state.capacity, .num_rendered, last_num_rendered()
PARENT_AFTER_RERUN = (_CAP, 20480, 9426, 1)          # the next frame: calls, state.capacity, .num_rendered, capacity_reruns gained so far
_FUSED_GRADS = "dL_dcolor dL_dmeans2D scratch_acc deform_epilogue scratch_acc_zeroed"
PARENT_GRADS_TWO_NODE = ["dL_dcolor dL_dmeans2D dL_dmeans3D dL_dopacity dL_dcolors dL_dsh dL_dscales dL_drotations dL_dcov3D scratch_acc scratch_acc_zeroed"]
PARENT_GRADS_FUSED = [_FUSED_GRADS]
PARENT_GRADS_VIEWS = [_FUSED_GRADS, _FUSED_GRADS, _FUSED_GRADS]


def test_a_speculative_frame_that_overflows_its_capacity_is_finished_exactly(fake):
    """BINNING = "auto": the second frame of a (size, count) key is queued for a predicted capacity; when its count proves larger, stages 3-4
    run again on a buffer of the true size before rasterize_forward returns, and the state describes THAT buffer."""
    R = fdgs.rasterizer
    assert R.BINNING == "auto"
    fake.record = True
    pc = _model(300)
    cam = _cam(0.5)
    settings = R.GaussianRasterizationSettings(48, 64, 0.36, 0.27, torch.zeros(3), 1.0, cam.world_view_transform, cam.full_proj_transform, 3,
                                               cam.camera_center, False, False)
    args = (settings, pc.get_xyz.detach(), torch.rand(300, 16, 3), None, torch.rand(300, 1), torch.rand(300, 3), torch.rand(300, 4), None)
    *_, first = R.rasterize_forward(*args)
    assert first.capacity == first.num_rendered == 7
    cap = (int(7 * R.CAPACITY_SLACK) + 8192) // 4096 * 4096
    fake.pair_count = cap + 1234
    fake.calls.clear()
    fake.pairs.clear()
    reruns = R.capacity_reruns
    *_, state = R.rasterize_forward(*args)
    assert " ".join(c[len("fdgs_"):] for c in fake.calls) == PARENT_RERUN_CALLS
    assert fake.pairs == PARENT_RERUN_PAIRS and fake.pairs[0][1] == cap and state.capacity == cap + 1234     # (the state's capacity is the true count)
    assert (R.capacity_reruns - reruns, R.capacity_overflows, state.capacity, state.num_rendered, R.last_num_rendered()) == PARENT_RERUN_STATE
    fake.calls.clear()                        # the predictor has learnt: the next frame fits
    *_, third = R.rasterize_forward(*args)
    assert (" ".join(c[len("fdgs_"):] for c in fake.calls), third.capacity, third.num_rendered, R.capacity_reruns - reruns) == PARENT_AFTER_RERUN


def test_raster_backwards_hand_over_the_gradient_buffers_they_handed_over_before(fake, monkeypatch):
    """Which fdgs_raster_grads pointers are non-NULL (and scratch_acc_zeroed): the two-node backward asks for every per-Gaussian gradient, the
    fused ones only for the screen-space means -- the rest goes through the deformation epilogue."""
    fake.record = True
    monkeypatch.setattr(fdgs.renderer, "FUSED_BACKWARD", False)
    _run_render_backward(fake, 300)
    assert fake.grads == PARENT_GRADS_TWO_NODE
    monkeypatch.setattr(fdgs.renderer, "FUSED_BACKWARD", True)
    fake.grads.clear()
    _run_render_backward(fake, 300)
    assert fake.grads == PARENT_GRADS_FUSED
    fake.grads.clear()
    fake.bwd_views.clear()
    _run_render_views(fake, 300)
    assert fake.grads == PARENT_GRADS_VIEWS
    # every view's deformation backward reads that view's own forward outputs (three views: twelve distinct buffers)
    assert len(fake.bwd_views) == 3 and len({q for view in fake.bwd_views for q in view}) == 12 and None not in fake.bwd_views[0]
