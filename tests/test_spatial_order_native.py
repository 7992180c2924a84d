"""The spatial order in the C-ABI, host side (no GPU): the four fdgs_spatial_* entry points are declared and bound, the scratch size query
works, and the library's key function -- evaluated on the HOST by fdgs_spatial_keys_host, the very function the device kernel compiles
(csrc/spatial_keys.h) -- equals fdgs.densify.hilbert_keys / morton_keys EXACTLY.  The torch expressions are the oracle; nothing here is a
tolerance."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

fdgs = importlib.import_module("4dgaussians_amd")
D = fdgs.densify
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fdgs_spatial_order_scratch_bytes", "fdgs_spatial_keys", "fdgs_spatial_order", "fdgs_spatial_keys_host")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(fdgs._lib.LIB_PATH):
        importlib.import_module("4dgaussians_amd.build").build()
    return fdgs._lib.lib()


def _host_keys(lib, xyz, bounds, curve, bits=10):
    x = np.ascontiguousarray(xyz.numpy(), dtype=np.float32)
    b = None if bounds is None else np.ascontiguousarray(np.asarray(bounds, dtype=np.float32).reshape(2, 3))
    keys = np.empty(max(x.shape[0], 1), dtype=np.uint32)
    rc = lib.fdgs_spatial_keys_host(x.shape[0], x.ctypes.data, None if b is None else b.ctypes.data, fdgs._lib.CURVES[curve], bits,
                                    keys.ctypes.data)
    assert rc == 0, lib.fdgs_last_error()
    return torch.from_numpy(keys[:x.shape[0]].astype(np.int64))


def test_header_declares_the_four_functions_and_lib_binds_them(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fdgs.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in fdgs._lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define\s+FDGS_CURVE_HILBERT\s+0\b", src) and re.search(r"#define\s+FDGS_CURVE_MORTON\s+1\b", src)
    assert fdgs._lib.CURVES == {"hilbert": 0, "morton": 1}
    assert lib.fdgs_abi_version() == 6


def test_scratch_bytes_answers_and_grows_monotonically(lib):
    n = ctypes.c_size_t()
    sizes = []
    for N in (0, 1, 300_000, 2_000_000):
        assert lib.fdgs_spatial_order_scratch_bytes(N, n) == 0
        sizes.append(n.value)
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[2] >= 300_000 * 12 and sizes[3] >= 2_000_000 * 12
    # ... also across the size at which the sort changes its workgroup size
    around = []
    for N in range((1 << 20) - 3, (1 << 20) + 4):
        assert lib.fdgs_spatial_order_scratch_bytes(N, n) == 0
        around.append(n.value)
    assert around == sorted(around)


def test_scratch_bytes_rejects_a_negative_count_with_a_message(lib):
    n = ctypes.c_size_t()
    assert lib.fdgs_spatial_order_scratch_bytes(-1, n) == -1
    assert b"bad" in lib.fdgs_last_error()


def test_bad_arguments_are_errors_with_a_message_and_zero_points_are_fine(lib):
    x = np.zeros((4, 3), np.float32)
    k = np.zeros(4, np.uint32)
    f = lib.fdgs_spatial_keys_host
    assert f(0, None, None, 0, 10, None) == 0                       # N = 0: nothing read, nothing written
    for args, word in (((-1, x.ctypes.data, None, 0, 10, k.ctypes.data), b"N"), ((4, x.ctypes.data, None, 0, 0, k.ctypes.data), b"bits"),
                       ((4, x.ctypes.data, None, 0, 11, k.ctypes.data), b"bits"), ((4, x.ctypes.data, None, 2, 10, k.ctypes.data), b"curve"),
                       ((4, None, None, 0, 10, k.ctypes.data), b"NULL"), ((4, x.ctypes.data, None, 0, 10, None), b"NULL")):
        assert f(*args) == -1, args
        assert word in lib.fdgs_last_error(), (args, lib.fdgs_last_error())
    # the device entry points check their arguments before they touch a device
    assert lib.fdgs_spatial_order(None, 4, None, None, 0, 10, None, None, None) == -1 and b"NULL" in lib.fdgs_last_error()
    assert lib.fdgs_spatial_keys(None, 4, x.ctypes.data, None, 1, 12, None, k.ctypes.data) == -1 and b"bits" in lib.fdgs_last_error()
    assert lib.fdgs_spatial_order(None, 0, None, None, 0, 10, None, None, None) == 0


@pytest.fixture(scope="module")
def cloud():
    return torch.randn(1_000_003, 3, generator=torch.Generator().manual_seed(11)) * 1.3


@pytest.mark.parametrize("curve", ["hilbert", "morton"])
def test_host_keys_equal_the_torch_keys_with_a_clamping_aabb(lib, cloud, curve):
    """An aabb of about +- 0.77 sigma per axis: more than half of the points are clamped on at least one axis.  The corners are passed as the
    train loop passes them (HexPlaneField.aabb: the "max" row first)."""
    hi, lo = [1.0, 0.9, 1.1], [-1.0, -1.1, -0.9]
    outside = ((cloud < torch.tensor(lo)) | (cloud > torch.tensor(hi))).any(1).float().mean()
    assert float(outside) > 0.5
    ref = (D.hilbert_keys if curve == "hilbert" else D.morton_keys)(cloud, lo, hi)
    assert torch.equal(_host_keys(lib, cloud, [hi, lo], curve), ref)
    assert torch.equal(_host_keys(lib, cloud, [lo, hi], curve), ref)              # either row order
    assert torch.equal(D.spatial_keys(cloud, lo, hi, curve=curve), ref)           # (CPU tensors: the torch path)


@pytest.mark.parametrize("curve", ["hilbert", "morton"])
@pytest.mark.parametrize("bits", [10, 7, 1])
def test_host_keys_equal_the_torch_keys_with_the_bounding_box(lib, cloud, curve, bits):
    ref = (D.hilbert_keys if curve == "hilbert" else D.morton_keys)(cloud, bits=bits)
    got = _host_keys(lib, cloud, None, curve, bits)
    assert torch.equal(got, ref)
    assert int(got.max()) < 1 << (3 * bits)


@pytest.mark.parametrize("curve", ["hilbert", "morton"])
def test_host_keys_of_identical_points(lib, curve):
    x = torch.full((5000, 3), 0.37)
    keyfn = D.hilbert_keys if curve == "hilbert" else D.morton_keys
    assert torch.equal(_host_keys(lib, x, None, curve), keyfn(x))
    assert torch.equal(_host_keys(lib, x, [[1.0, 1, 1], [-1.0, -1, -1]], curve), keyfn(x, [-1.0, -1, -1], [1.0, 1, 1]))
    assert torch.unique(_host_keys(lib, x, None, curve)).numel() == 1


@pytest.mark.parametrize("curve", ["hilbert", "morton"])
def test_host_keys_are_a_bijection_on_the_cell_centres_of_an_8_cubed_grid(lib, curve):
    b = 3
    g = torch.stack(torch.meshgrid(*[torch.arange(2 ** b)] * 3, indexing="ij"), -1).reshape(-1, 3).float() + 0.5
    got = _host_keys(lib, g, [[0.0, 0, 0], [8.0, 8, 8]], curve, bits=b)
    assert torch.equal(got, (D.hilbert_keys if curve == "hilbert" else D.morton_keys)(g, [0, 0, 0], [8, 8, 8], bits=b))
    assert torch.unique(got).numel() == g.shape[0] == 512
    if curve == "hilbert":          # consecutive cells along the curve are face neighbours
        order = torch.argsort(got)
        assert torch.all((g[order][1:] - g[order][:-1]).abs().sum(1) == 1.0)


def test_non_finite_coordinates_go_to_cell_zero_of_their_axis(lib):
    x = torch.tensor([[0.25, 0.5, 0.75], [float("nan"), 0.5, 0.75], [0.25, float("inf"), 0.75], [0.25, 0.5, float("-inf")]])
    box = [[0.0, 0, 0], [1.0, 1, 1]]
    got = _host_keys(lib, x, box, "morton")
    ref = D.morton_keys(torch.tensor([[0.25, 0.5, 0.75], [0.0, 0.5, 0.75], [0.25, 0.0, 0.75], [0.25, 0.5, 0.0]]), [0, 0, 0], [1, 1, 1])
    assert torch.equal(got, ref)
    # ... and stay out of the bounding box
    y = torch.cat([torch.rand(100, 3, generator=torch.Generator().manual_seed(2)), torch.tensor([[float("inf"), float("nan"), 0.5]])])
    assert torch.equal(_host_keys(lib, y, None, "hilbert")[:100], D.hilbert_keys(y[:100], y[:100].min(0).values, y[:100].max(0).values))


def test_spatial_order_on_cpu_tensors_is_the_stable_argsort_of_the_torch_keys(cloud):
    x = cloud[:200_000].clone()
    x[1000:3000] = x[0]                                     # ties: the stable order is unique, an unstable one is not
    perm = D.spatial_order(x)
    assert perm.dtype == torch.int32 and perm.device == x.device
    assert torch.equal(perm.long(), torch.argsort(D.hilbert_keys(x), stable=True))
    lo, hi = [-1.0, -1, -1], [1.0, 1, 1]
    assert torch.equal(D.spatial_order(x, lo, hi, curve="morton").long(), torch.argsort(D.morton_keys(x, lo, hi), stable=True))
    assert torch.equal(D.spatial_order(x, lo, hi, bits=4).long(), torch.argsort(D.hilbert_keys(x, lo, hi, bits=4), stable=True))
    with pytest.raises(ValueError):
        D.spatial_order(x, curve="peano")


def test_implicit_perm_is_none_for_a_half_precision_sh_tensor():
    """render() reads an unordered model through fdgs_permute_rows, which moves rows of 4-byte elements: a model with a float16 SH tensor
    must take the unpermuted path (which accepts it) instead of raising inside permute_rows."""
    syn, R = fdgs.synthetic, fdgs.renderer
    n = 8192
    pc = syn.SynthModel(n, "dynerf_default", seed=3)
    dn = pc._deformation.deformation_net
    fdgs.deformation.invalidate_caches()
    perm = R._implicit_perm(pc, {"ordered": False}, dn)
    assert perm is not None and perm.dtype == torch.int32 and sorted(perm.tolist()) == list(range(n))
    aabb = dn.grid.aabb
    assert torch.equal(perm.long(), torch.argsort(D.hilbert_keys(pc._xyz, aabb[1], aabb[0]), stable=True))
    half = syn.SynthModel(n, "dynerf_default", seed=3)
    half._features_rest = torch.nn.Parameter(half._features_rest.detach().half())
    assert R._implicit_perm(half, {"ordered": False}, half._deformation.deformation_net) is None
    assert R._implicit_perm(pc, {"ordered": True}, dn) is None          # (an ordered set needs none, as before)
