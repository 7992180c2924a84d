"""Host-side (no GPU) checks of sparse Adam: the arithmetic and the row-mask walk of csrc/adam.hip through fdgs_adam_step_rows_host (the
same rows_live / adam1 the device kernel calls), the C ABI's refusals, and SparseGaussianAdam's optimizer surface and Python refusals.
Cases, references and the error measure are in sparse_adam_common.py.

Per-element bound |x - x64| <= c * 2^-23 * (|x64| + |dx64|) with c = max(1, 2 * torch's worst ratio).  Measured worst ratios over the 21
cases (N in {1, 33, 1001} x seven first masks, six steps each), for (p, exp_avg, exp_avg_sq):

    bias_correction=True     torch float32 CPU Adam  (1.53, 0.60, 1.05)  ->  c = 3.06     host twin (1.90, 0.93, 1.05)
    bias_correction=False    torch float32 formulas  (1.58, 0.60, 1.05)  ->  c = 3.17     host twin (2.43, 0.93, 1.05)

(The host twin takes the learning rate as a float and divides m by the denominator before it scales, torch keeps the learning rate a double
and scales inside addcdiv: two correct float32 evaluations.)  The device figures are in test_gpu_sparse_adam.py.
"""
import ctypes
import importlib

import pytest
import torch

import sparse_adam_common as C

fdgs = importlib.import_module("4dgaussians_amd")
L = fdgs._lib


@pytest.fixture(scope="module")
def lib():
    return L.lib()


def descriptors(chain, it, vis, step=None):
    """One fdgs_adam_rows_tensor per tensor of the chain at step `it`; `vis` is the uint8 / bool mask tensor the row groups point at."""
    g = chain.grads(it)
    lrs = chain.steps[it][1]
    ds = []
    for k in chain.names:
        d = L.AdamRowsTensor()
        d.param, d.grad, d.exp_avg, d.exp_avg_sq = chain.p[k].data_ptr(), g[k].data_ptr(), chain.m[k].data_ptr(), chain.v[k].data_ptr()
        if k in C.ROW_GROUPS:
            d.rows, d.row_len, d.visible = chain.N, chain.p[k].numel() // chain.N, vis.data_ptr()
        else:
            d.rows, d.row_len, d.visible = chain.p[k].numel(), 1, None
        d.lr, d.step = lrs[k], (it + 1 if step is None else step)
        ds.append(d)
    return (L.AdamRowsTensor * len(ds))(*ds), g


def run_host_chain(lib, N, first, bias_correction, poison=False):
    chain = C.Chain(N, first, torch.device("cpu"), poison)
    c = C.bound_c(bias_correction)
    for it in range(C.STEPS):
        vis = chain.steps[it][2].to(torch.uint8)
        arr, keep = descriptors(chain, it, vis)
        before = chain.snapshot()
        L.check(lib.fdgs_adam_step_rows_host(len(arr), arr, *C.BETAS, C.EPS, int(bias_correction)))
        chain.check_step(it, before, bias_correction, c)
    chain.check_against_reference(bias_correction)
    return chain.worst


@pytest.mark.parametrize("bias_correction", [True, False])
@pytest.mark.parametrize("N,first", C.cases())
def test_host_twin_steps_visible_rows_only_within_the_float64_bound(lib, N, first, bias_correction):
    worst = run_host_chain(lib, N, first, bias_correction)
    print(f"N={N} first={C.MASK_KINDS[first]} bias_correction={bias_correction}: host twin worst ratio {worst}, "
          f"torch {C.torch_ratios(bias_correction)}, c = {C.bound_c(bias_correction)}")


@pytest.mark.parametrize("first", [0, 4, 6])
def test_nan_and_inf_in_invisible_gradients_change_nothing(lib, first):
    run_host_chain(lib, 1001, first, True, poison=True)
    run_host_chain(lib, 33, first, False, poison=True)


def test_seventy_masked_tensors_cross_the_chunk_of_64(lib):
    N, T = 33, 70
    gen = torch.Generator().manual_seed(7)
    vis = C.make_mask("alternate", N).to(torch.uint8)
    rows = vis.bool()
    p = [torch.randn(N, 1 + i % 5, generator=gen) for i in range(T)]
    g = [torch.randn(N, 1 + i % 5, generator=gen) for i in range(T)]
    m = [torch.randn(N, 1 + i % 5, generator=gen) * 0.1 for i in range(T)]
    v = [torch.rand(N, 1 + i % 5, generator=gen) for i in range(T)]
    before = [(a.clone(), b.clone(), c.clone()) for a, b, c in zip(p, m, v)]
    arr = (L.AdamRowsTensor * T)()
    for i in range(T):
        arr[i].param, arr[i].grad, arr[i].exp_avg, arr[i].exp_avg_sq = p[i].data_ptr(), g[i].data_ptr(), m[i].data_ptr(), v[i].data_ptr()
        arr[i].rows, arr[i].row_len, arr[i].visible, arr[i].lr, arr[i].step = N, 1 + i % 5, vis.data_ptr(), 1e-3 * (1 + i), 1 + i % 3
    L.check(lib.fdgs_adam_step_rows_host(T, arr, *C.BETAS, C.EPS, 1))
    c = C.bound_c(True)
    for i in range(T):
        x64 = C.f64_step(*before[i], g[i], 1e-3 * (1 + i), 1 + i % 3, rows, True)
        for new, ref, old in zip((p[i], m[i], v[i]), x64, before[i]):
            assert C.same_bits(new[~rows], old[~rows]), i
            assert not C.same_bits(new[rows], old[rows]), i
            assert C.ratio(new, ref, old, rows) <= c, i


def _one(n=8, row_len=2):
    t = [torch.zeros(n * row_len) for _ in range(4)]
    vis = torch.ones(n, dtype=torch.uint8)
    arr = (L.AdamRowsTensor * 1)()
    arr[0].param, arr[0].grad, arr[0].exp_avg, arr[0].exp_avg_sq = (x.data_ptr() for x in t)
    arr[0].rows, arr[0].row_len, arr[0].visible, arr[0].lr, arr[0].step = n, row_len, vis.data_ptr(), 0.1, 1
    return arr, t, vis


def test_abi_refusals_and_no_ops(lib):
    call = lambda arr, n=1: lib.fdgs_adam_step_rows_host(n, arr, 0.9, 0.999, 1e-15, 1)
    arr, t, vis = _one()
    assert call(arr) == 0
    arr[0].step = 0
    assert call(arr) != 0 and b"step counts from 1" in lib.fdgs_last_error()
    arr, t, vis = _one()
    arr[0].row_len = 0
    assert call(arr) != 0 and b"row_len" in lib.fdgs_last_error()
    for field in ("param", "grad", "exp_avg", "exp_avg_sq"):
        arr, t, vis = _one()
        setattr(arr[0], field, None)
        assert call(arr) != 0 and b"NULL" in lib.fdgs_last_error(), field
        arr, t, vis = _one()
        setattr(arr[0], field, getattr(arr[0], field) + 4)
        assert call(arr) != 0 and b"aligned" in lib.fdgs_last_error(), field
    arr, t, vis = _one()
    arr[0].rows, arr[0].row_len = 2 ** 31, 2            # refused on its sizes, before any element is touched
    assert call(arr) != 0 and b"too large" in lib.fdgs_last_error()
    arr[0].rows, arr[0].row_len = 2 ** 32, 1
    assert call(arr) != 0 and b"too large" in lib.fdgs_last_error()
    assert call(None) != 0 and b"bad tensor list" in lib.fdgs_last_error()
    # a refused list has stepped nothing: the good tensor in front of a bad one is untouched
    arr2 = (L.AdamRowsTensor * 2)()
    good, t, vis = _one()
    t[1].fill_(1.0)                                      # a gradient that would move the parameter
    bad, t_bad, vis_bad = _one()
    bad[0].step = 0
    ctypes.memmove(ctypes.byref(arr2, 0), ctypes.byref(good), ctypes.sizeof(L.AdamRowsTensor))
    ctypes.memmove(ctypes.byref(arr2, ctypes.sizeof(L.AdamRowsTensor)), ctypes.byref(bad), ctypes.sizeof(L.AdamRowsTensor))
    assert call(arr2, 2) != 0 and float(t[0].abs().sum()) == 0.0
    # no-ops: an empty list (with or without an array) and a tensor of zero rows (its other fields are not looked at)
    assert call(None, 0) == 0 and call(arr, 0) == 0
    empty = (L.AdamRowsTensor * 1)()
    assert call(empty) == 0
    # the device entry point refuses the same descriptors before it touches a stream
    arr, t, vis = _one()
    arr[0].step = 0
    assert lib.fdgs_adam_step_rows(None, 1, arr, 0.9, 0.999, 1e-15, 1) != 0 and b"step counts from 1" in lib.fdgs_last_error()
    assert lib.fdgs_adam_step_rows(None, 0, None, 0.9, 0.999, 1e-15, 1) == 0


def test_dense_descriptor_without_a_mask_steps_every_element(lib):
    arr, t, vis = _one(n=7, row_len=1)
    arr[0].visible = None
    t[1].fill_(2.0)
    assert lib.fdgs_adam_step_rows_host(1, arr, 0.9, 0.999, 1e-15, 1) == 0
    assert bool((t[0] < 0).all()) and bool((t[2] > 0).all()) and bool((t[3] > 0).all())


# ---- SparseGaussianAdam: optimizer surface and Python refusals (CPU tensors: nothing here reaches a kernel) ------------------------------
def _groups(N=5):
    a, b, w = torch.nn.Parameter(torch.rand(N, 3)), torch.nn.Parameter(torch.rand(N, 1)), torch.nn.Parameter(torch.rand(4, 4))
    return [{"params": [a], "lr": 1e-3, "name": "xyz"}, {"params": [b], "lr": 0.0, "name": "opacity"},
            {"params": [w], "lr": 1e-4, "name": "deformation"}], (a, b, w)


def test_class_structure_matches_torch_adam_and_loads_its_checkpoint():
    g1, (a, b, w) = _groups()
    opt = fdgs.SparseGaussianAdam(g1, lr=0.0, eps=1e-15)
    ref = torch.optim.Adam(_groups()[0], lr=0.0, eps=1e-15)
    assert isinstance(opt, fdgs.FusedAdam) and isinstance(opt, torch.optim.Optimizer)
    assert opt.row_groups == C.ROW_GROUPS and opt.bias_correction is True
    assert "SparseGaussianAdam" in fdgs.__all__ and "SparseGaussianAdam" in fdgs.__doc__
    fused = fdgs.FusedAdam(_groups()[0], lr=0.0, eps=1e-15)
    for go, gr, gf in zip(opt.param_groups, ref.param_groups, fused.param_groups):
        assert set(go) == set(gf) and set(go) <= set(gr)      # FusedAdam's keys, each of them one of torch.optim.Adam's
        for k in ("lr", "betas", "eps", "weight_decay", "amsgrad", "name"):
            assert go[k] == gr[k], k
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and sd["state"] == {}
    g2, ps = _groups()
    ref2 = torch.optim.Adam(g2, lr=0.0, eps=1e-15)
    for p in ps:
        p.grad = torch.ones_like(p)
    ref2.step()
    opt.load_state_dict(ref2.state_dict())
    st = opt.state[a]
    assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 1.0
    assert set(opt.state_dict()["state"][0]) == set(ref2.state_dict()["state"][0])
    with pytest.raises(NotImplementedError):
        fdgs.SparseGaussianAdam(_groups()[0], weight_decay=0.1)
    with pytest.raises(NotImplementedError):
        fdgs.SparseGaussianAdam(_groups()[0], amsgrad=True)
    assert fdgs.SparseGaussianAdam(_groups()[0], row_groups=("xyz",), bias_correction=False).row_groups == ("xyz",)


def test_python_refusals_come_before_any_launch():
    N = 5
    groups, (a, b, w) = _groups(N)
    opt = fdgs.SparseGaussianAdam(groups, lr=0.0, eps=1e-15)
    for p in (a, b, w):
        p.grad = torch.ones_like(p)
    ok = torch.ones(N, dtype=torch.bool)
    bad_masks = [torch.ones(N), torch.ones(N, dtype=torch.int32), torch.ones(N, 1, dtype=torch.bool), torch.ones(2 * N, dtype=torch.uint8)[::2],
                 torch.ones(N + 1, dtype=torch.bool), torch.ones(N, dtype=torch.bool, device="meta"), [True] * N]
    for m in bad_masks:
        with pytest.raises(ValueError):
            opt.step(m)
    with pytest.raises(ValueError):
        opt.step(ok, N + 1)                              # N disagrees with the mask
    with pytest.raises(ValueError):
        opt.step(None, N)                                # N without a mask
    # a row-group parameter that is not row-major contiguous
    groups, (a, b, w) = _groups(N)
    groups[0]["params"][0] = t = torch.nn.Parameter(torch.rand(3, N).t())
    opt2 = fdgs.SparseGaussianAdam(groups, lr=0.0, eps=1e-15)
    t.grad = torch.ones_like(t)
    with pytest.raises(ValueError, match="contiguous"):
        opt2.step(ok, N)
    # none of the refusals counted a step or made state
    assert len(opt.state) == 0 and len(opt2.state) == 0
    # with everything about the mask in order the FusedAdam refusals follow: CPU tensors have no kernel
    with pytest.raises(L.FdgsError):
        opt.step(ok, N)
    with pytest.raises(L.FdgsError):
        opt.step(ok.to(torch.uint8))
    with pytest.raises(L.FdgsError):
        opt.step()
    # non-float32 and sparse gradients are refused as FusedAdam refuses them
    h = torch.nn.Parameter(torch.rand(N, 3, dtype=torch.float64))
    opt3 = fdgs.SparseGaussianAdam([{"params": [h], "name": "xyz"}], lr=0.0, eps=1e-15)
    h.grad = torch.ones_like(h)
    with pytest.raises(L.FdgsError):
        opt3.step(ok, N)
