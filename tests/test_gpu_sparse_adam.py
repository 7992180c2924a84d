"""GPU checks of sparse Adam: the cases of sparse_adam_common.py through fdgs_adam_step_rows (adam_kernel<true, AdamRowsArgs> of
csrc/adam.hip) and through SparseGaussianAdam.step(visibility, N), with the bounds and the exactness of the host test
(test_sparse_adam_host.py): invisible rows bit-identical, stepped elements within c * 2^-23 * (|x64| + |dx64|) of float64, c = twice what
torch's float32 CPU Adam reaches.  Then what the dense instantiation shares with it (visibility=None == all-ones mask == FusedAdam,
torch.equal), bool == uint8 masks, the densification state surgery, prune_points, and a mask left on the host.

Measured worst ratios of the device (MI355X) over the 21 cases, (p, exp_avg, exp_avg_sq): (1.90, 0.71, 0.90) with the bias corrections
against c = 3.06, (1.90, 0.71, 0.90) without against c = 3.17.
"""
import importlib

import pytest
import torch

import sparse_adam_common as C
from test_sparse_adam_host import descriptors

pytestmark = pytest.mark.gpu
fdgs = importlib.import_module("4dgaussians_amd")
L = fdgs._lib
DEV = torch.device("cuda:0")


def _on_device(*tensors):
    for t in tensors:
        assert t.is_cuda and t.device == DEV, "a host tensor must never reach a kernel"


@pytest.mark.parametrize("bias_correction", [True, False])
@pytest.mark.parametrize("N,first", C.cases())
def test_abi_steps_visible_rows_only_within_the_float64_bound(N, first, bias_correction):
    lib = L.lib()
    chain = C.Chain(N, first, DEV)
    c = C.bound_c(bias_correction)
    for it in range(C.STEPS):
        vis = chain.steps[it][2].to(DEV).view(torch.uint8)
        arr, keep = descriptors(chain, it, vis)
        _on_device(vis, *keep.values(), *chain.p.values(), *chain.m.values(), *chain.v.values())
        before = chain.snapshot()
        L.check(lib.fdgs_adam_step_rows(L.stream_ptr(), len(arr), arr, *C.BETAS, C.EPS, int(bias_correction)))
        torch.cuda.synchronize()
        chain.check_step(it, before, bias_correction, c)
    chain.check_against_reference(bias_correction)
    print(f"N={N} first={C.MASK_KINDS[first]} bias_correction={bias_correction}: device worst ratio {chain.worst}, c = {c}")


def _optimizer(chain, cls=None, **kw):
    """The chain's tensors as Parameters of an optimizer whose state IS the chain's moments (what load_state_dict / densify leave)."""
    params = {k: torch.nn.Parameter(chain.p[k]) for k in chain.p}
    opt = (cls or fdgs.SparseGaussianAdam)([{"params": [params[k]], "lr": 0.0, "name": k} for k in params], lr=0.0, eps=C.EPS, betas=C.BETAS, **kw)
    for k in chain.names:
        opt.state[params[k]] = {"step": torch.tensor(0.0), "exp_avg": chain.m[k], "exp_avg_sq": chain.v[k]}
    return opt, params


def _set(opt, params, chain, it):
    g = chain.grads(it)
    for group in opt.param_groups:
        group["lr"] = chain.steps[it][1][group["name"]]
    for k in chain.names:
        params[k].grad = g[k]


@pytest.mark.parametrize("bias_correction,poison", [(True, False), (False, False), (True, True)])
@pytest.mark.parametrize("N,first", [(1001, 0), (1001, 3), (1001, 6), (33, 2), (1, 1)])
def test_class_steps_visible_rows_only_within_the_float64_bound(N, first, bias_correction, poison):
    chain = C.Chain(N, first, DEV, poison)
    opt, params = _optimizer(chain, bias_correction=bias_correction)
    c = C.bound_c(bias_correction)
    for it in range(C.STEPS):
        _set(opt, params, chain, it)
        before = chain.snapshot()
        mask = chain.steps[it][2].to(DEV)
        opt.step(mask, N)
        torch.cuda.synchronize()
        chain.check_step(it, before, bias_correction, c)
        assert float(opt.state[params["xyz"]]["step"]) == it + 1.0          # calls per tensor, not visits per row
    chain.check_against_reference(bias_correction)
    assert len(opt.state[params["unused"]]) == 0
    assert chain.p["plane"].is_contiguous(memory_format=torch.channels_last)


def test_no_mask_all_ones_mask_and_fused_adam_are_the_same_bits():
    runs = {}
    for name in ("fused", "none", "ones_bool", "ones_u8"):
        chain = C.Chain(1001, 1, DEV)
        opt, params = _optimizer(chain, fdgs.FusedAdam if name == "fused" else fdgs.SparseGaussianAdam)
        for it in range(3):
            _set(opt, params, chain, it)
            if name == "fused":
                opt.step()
            elif name == "none":
                opt.step(None)
            else:
                opt.step(torch.ones(1001, device=DEV, dtype=torch.bool if name == "ones_bool" else torch.uint8), 1001)
        torch.cuda.synchronize()
        runs[name] = chain
    for name in ("none", "ones_bool", "ones_u8"):
        for k in runs["fused"].names:
            for a, b in zip((runs[name].p[k], runs[name].m[k], runs[name].v[k]), (runs["fused"].p[k], runs["fused"].m[k], runs["fused"].v[k])):
                assert torch.equal(a, b), (name, k)


def test_bool_and_uint8_masks_give_equal_bits():
    runs = []
    for dtype in (torch.bool, torch.uint8):
        chain = C.Chain(1001, 4, DEV)
        opt, params = _optimizer(chain)
        for it in range(3):
            _set(opt, params, chain, it)
            mask = chain.steps[it][2].to(DEV)
            opt.step(mask if dtype == torch.bool else mask.to(torch.uint8) * 255, 1001)        # any nonzero byte is "visible"
        torch.cuda.synchronize()
        runs.append(chain)
    for k in runs[0].names:
        for a, b in zip((runs[0].p[k], runs[0].m[k], runs[0].v[k]), (runs[1].p[k], runs[1].m[k], runs[1].v[k])):
            assert torch.equal(a, b), k


def test_state_surgery_then_sparse_steps_against_the_yardstick():
    """The surgery of test_gpu_optim.py::test_state_surgery_and_state_dict_round_trip (new Parameter, sliced state, re-keyed, state_dict
    round trip) on a SparseGaussianAdam, then two sparse steps at the new N against torch.optim.Adam with the invisible rows put back."""
    gen = torch.Generator().manual_seed(1)
    sh = C.shapes(1001)
    cpu = {k: torch.nn.Parameter(torch.randn(*s, generator=gen)) for k, s in sh.items()}
    gpu = {k: torch.nn.Parameter(v.detach().clone().to(DEV)) for k, v in cpu.items()}
    gpu["plane"] = torch.nn.Parameter(gpu["plane"].detach().contiguous(memory_format=torch.channels_last))
    groups = lambda d: [{"params": [d[k]], "lr": 1e-3 * (i + 1), "name": k} for i, k in enumerate(sh)]
    ref = torch.optim.Adam(groups(cpu), lr=0.0, eps=C.EPS)
    opt = fdgs.SparseGaussianAdam(groups(gpu), lr=0.0, eps=C.EPS)

    def set_grads():
        for k in cpu:
            if k != "unused":
                g = torch.randn(cpu[k].shape, generator=gen)
                cpu[k].grad, gpu[k].grad = g.clone(), g.to(DEV)

    def sparse_ref_step(vis):
        before = {k: (cpu[k].detach().clone(), ref.state[cpu[k]]["exp_avg"].clone(), ref.state[cpu[k]]["exp_avg_sq"].clone()) for k in C.ROW_GROUPS}
        ref.step()
        with torch.no_grad():
            for k in C.ROW_GROUPS:
                for new, old in zip((cpu[k], ref.state[cpu[k]]["exp_avg"], ref.state[cpu[k]]["exp_avg_sq"]), before[k]):
                    new[~vis] = old[~vis]

    set_grads()
    ref.step(); opt.step()
    mask = torch.rand(1001, generator=gen) > 0.3
    for o, params in ((ref, cpu), (opt, gpu)):
        for group in o.param_groups:
            if group["name"] not in C.ROW_GROUPS:
                continue
            old = group["params"][0]
            m = mask.to(old.device)
            st = o.state.get(old, None)
            st["exp_avg"] = st["exp_avg"][m]
            st["exp_avg_sq"] = st["exp_avg_sq"][m]
            del o.state[old]
            group["params"][0] = torch.nn.Parameter(old[m].detach().requires_grad_(True))
            o.state[group["params"][0]] = st
            params[group["name"]] = group["params"][0]
    sd = opt.state_dict()
    opt2 = fdgs.SparseGaussianAdam([{"params": [gpu[g["name"]]], "lr": g["lr"], "name": g["name"]} for g in opt.param_groups], lr=0.0, eps=C.EPS)
    opt2.load_state_dict(sd)
    n2 = int(mask.sum())
    for it in range(2):
        set_grads()
        vis = torch.rand(n2, generator=gen) < 0.4
        sparse_ref_step(vis)
        before = {k: gpu[k].detach().cpu().clone() for k in C.ROW_GROUPS}
        opt2.step(vis.to(DEV), n2)
        torch.cuda.synchronize()
        for k in C.ROW_GROUPS:
            assert C.same_bits(gpu[k].detach().cpu()[~vis], before[k][~vis]), k
    for k in cpu:
        assert gpu[k].shape == cpu[k].shape
        assert C.rel_l2(gpu[k].detach().cpu().numpy(), cpu[k].detach().numpy()) < 1e-6, k
        if k != "unused":
            for key in ("exp_avg", "exp_avg_sq"):
                assert C.rel_l2(opt2.state[gpu[k]][key].cpu().numpy(), ref.state[cpu[k]][key].numpy()) < 1e-6, (k, key)
    assert float(opt2.state[gpu["xyz"]]["step"]) == 3.0


def test_prune_points_then_a_sparse_step_at_the_new_n():
    n = 257
    pc = fdgs.synthetic.SynthModel(n, "dynerf_default", seed=5).to(DEV)
    pc.optimizer = fdgs.SparseGaussianAdam(pc.optimizer_groups(lr=1e-3), lr=0.0, eps=C.EPS)
    gen = torch.Generator().manual_seed(3)
    pc.xyz_gradient_accum, pc.denom = torch.zeros(n, 1, device=DEV), torch.zeros(n, 1, device=DEV)
    pc.max_radii2D, pc._deformation_accum = torch.zeros(n, device=DEV), torch.zeros(n, 3, device=DEV)
    pc._deformation_table = torch.ones(n, dtype=torch.bool, device=DEV)
    names = dict(fdgs.densify.ATTR)
    for a in names.values():
        p = getattr(pc, a)
        p.grad = torch.randn(p.shape, generator=gen).to(DEV)
    pc.optimizer.step(torch.ones(n, dtype=torch.bool, device=DEV), n)            # makes the moments the surgery slices
    drop = torch.rand(n, generator=gen) < 0.25
    fdgs.densify.prune_points(pc, drop.to(DEV), reorder=False)
    n2 = n - int(drop.sum())
    assert pc._xyz.shape[0] == n2
    vis = torch.rand(n2, generator=gen) < 0.5
    before = {}
    for k, a in names.items():
        p = getattr(pc, a)
        assert p.shape[0] == n2 and pc.optimizer.state[p]["exp_avg"].shape == p.shape
        p.grad = torch.randn(p.shape, generator=gen).to(DEV)
        st = pc.optimizer.state[p]
        before[k] = tuple(x.detach().cpu().clone() for x in (p, st["exp_avg"], st["exp_avg_sq"]))
    pc.optimizer.step(vis.to(DEV), n2)
    torch.cuda.synchronize()
    c = C.bound_c(True)
    for k, a in names.items():
        p = getattr(pc, a)
        st = pc.optimizer.state[p]
        assert float(st["step"]) == 2.0
        x64 = C.f64_step(*before[k], p.grad, 1e-3, 2, vis, True)
        for new, ref, old in zip((p, st["exp_avg"], st["exp_avg_sq"]), x64, before[k]):
            new = new.detach().cpu()
            assert C.same_bits(new[~vis], old[~vis]), k
            assert C.ratio(new, ref, old, vis) <= c, k
    with pytest.raises(ValueError):
        pc.optimizer.step(torch.ones(n, dtype=torch.bool, device=DEV), n)        # the mask of the old N


def test_a_mask_left_on_the_host_raises_and_launches_nothing():
    chain = C.Chain(33, 1, DEV)
    opt, params = _optimizer(chain)
    _set(opt, params, chain, 0)
    before = chain.snapshot()
    with pytest.raises(ValueError):
        opt.step(torch.ones(33, dtype=torch.bool), 33)
    torch.cuda.synchronize()
    after = chain.snapshot()
    for k in chain.names:
        for a, b in zip(before[k], after[k]):
            assert C.same_bits(a, b), k
    assert float(opt.state[params["xyz"]]["step"]) == 0.0
