"""Drop-in for the reference's optimizer (`torch.optim.Adam(l, lr=0.0, eps=1e-15)`, scene/gaussian_model.py:184;
stepped at train.py:291): the same `torch.optim.Optimizer` surface -- `param_groups` with per-group "lr"/"name" that
`update_learning_rate` (scene/gaussian_model.py:198-212) rewrites every iteration, and a per-parameter `state` dict with
the keys "step", "exp_avg", "exp_avg_sq" that the densification code edits in place (`replace_tensor_to_optimizer`,
`_prune_optimizer`, `cat_tensors_to_optimizer`, :316-400) and that `state_dict()` / `load_state_dict()` persist in
checkpoints -- but `step()` is ONE multi-tensor HIP launch (csrc/adam.hip) instead of ~5 elementwise kernels per tensor.

    self.optimizer = fdgs.FusedAdam(l, lr=0.0, eps=1e-15)        # scene/gaussian_model.py:184

`SparseGaussianAdam` is the same optimizer stepping only the Gaussians a frame saw (graphdeco's `SparseGaussianAdam`,
gsplat's `SelectiveAdam`): rows of the per-Gaussian tensors whose `visibility` is 0 keep their value and both moments bit
for bit, every other tensor is stepped densely, all in the same single launch.

    self.optimizer = fdgs.SparseGaussianAdam(l, lr=0.0, eps=1e-15)
    gaussians.optimizer.step(visibility_filter, visibility_filter.shape[0])      # train.py:291
"""
import torch

from . import _lib
from ._lib import AdamRowsTensor, AdamTensor, check, stream_ptr

ROW_GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        if weight_decay != 0 or amsgrad:
            raise NotImplementedError("FusedAdam implements the reference's configuration: no weight decay, no amsgrad")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._launch()
        return loss

    def _launch(self, visibility=None, row_groups=(), bias_correction=True):
        """One launch per distinct (beta1, beta2, eps) over every parameter with a gradient.  `visibility` (already checked by the caller)
        masks the rows of the groups named in `row_groups`; without a mask and with the bias corrections this is fdgs_adam_step."""
        L = _lib.lib()
        rows_form = visibility is not None or not bias_correction
        buckets = {}   # (beta1, beta2, eps) -> list of descriptors; one launch per distinct hyper-parameter set
        keep = []
        Descriptor = AdamRowsTensor if rows_form else AdamTensor
        for group in self.param_groups:
            b1, b2 = group["betas"]
            bucket, lr = None, float(group["lr"])       # (per group, not per tensor: this loop is host time of every training step)
            masked = visibility is not None and group.get("name") in row_groups
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.device.type != "cuda" or p.dtype != torch.float32:
                    raise _lib.FdgsError("FusedAdam steps float32 parameters on the GPU only")
                if p.grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                g, m, v = p.grad, st["exp_avg"], st["exp_avg_sq"]
                # one flat walk over memory: all four tensors must be dense with the same strides
                if not _dense(p):
                    raise _lib.FdgsError("FusedAdam needs dense (non-overlapping) parameters")
                if g.stride() != p.stride():
                    g = torch.empty_like(p, memory_format=torch.preserve_format).copy_(g)
                if m.stride() != p.stride():
                    m = st["exp_avg"] = torch.empty_like(p, memory_format=torch.preserve_format).copy_(m)
                if v.stride() != p.stride():
                    v = st["exp_avg_sq"] = torch.empty_like(p, memory_format=torch.preserve_format).copy_(v)
                st["step"] += 1
                d = Descriptor()
                d.param, d.grad, d.exp_avg, d.exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
                if not rows_form:
                    d.n, d.lr, d.step = p.numel(), lr, int(st["step"])
                elif masked:      # [N, row_len] in memory (row-major contiguous, checked by the caller); the mask is read in place
                    d.rows, d.row_len, d.visible = p.shape[0], max(p.numel() // max(p.shape[0], 1), 1), visibility.data_ptr()
                    d.lr, d.step = lr, int(st["step"])
                else:
                    d.rows, d.row_len, d.visible, d.lr, d.step = p.numel(), 1, None, lr, int(st["step"])
                if bucket is None:
                    bucket = buckets.setdefault((float(b1), float(b2), float(group["eps"])), [])
                bucket.append(d)
                keep.append((g, m, v))
        for (b1, b2, eps), ds in buckets.items():
            if rows_form:
                arr = (AdamRowsTensor * len(ds))(*ds)
                check(L.fdgs_adam_step_rows(stream_ptr(), len(ds), arr, b1, b2, eps, int(bool(bias_correction))))
            else:
                arr = (AdamTensor * len(ds))(*ds)
                check(L.fdgs_adam_step(stream_ptr(), len(ds), arr, b1, b2, eps))


class SparseGaussianAdam(FusedAdam):
    """FusedAdam that steps only the visible rows of the per-Gaussian tensors: `step(visibility_filter, N)`.

    `row_groups` names the param groups whose tensors are [N, ...] (the six of GaussianModel.training_setup); every other group
    (deformation, grid) is stepped densely.  `state[p]["step"]` counts calls per tensor, and the bias corrections use that count;
    `bias_correction=False` gives the upstream kernels' uncorrected form.  `step()` without a mask is FusedAdam.step()."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, row_groups=ROW_GROUPS,
                 bias_correction=True):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        self.row_groups = tuple(row_groups)
        self.bias_correction = bool(bias_correction)

    @torch.no_grad()
    def step(self, visibility=None, N=None, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if visibility is not None:
            self._check_mask(visibility, N)
        elif N is not None:
            raise ValueError("N without a visibility mask")
        self._launch(visibility, self.row_groups, self.bias_correction)
        return loss

    def _check_mask(self, visibility, N):
        """Everything about the mask and the tensors it masks that the kernel takes on trust -- refused here, before any launch."""
        if not isinstance(visibility, torch.Tensor) or visibility.dtype not in (torch.bool, torch.uint8):
            raise ValueError("visibility must be a bool or uint8 tensor")
        if visibility.dim() != 1 or not visibility.is_contiguous():
            raise ValueError("visibility must be a contiguous 1-D tensor [N]")
        if N is not None and int(N) != visibility.numel():
            raise ValueError(f"N = {N} but visibility has {visibility.numel()} rows")
        for group in self.param_groups:
            if group.get("name") not in self.row_groups:
                continue
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.device != visibility.device:
                    raise ValueError(f"visibility is on {visibility.device}, the '{group['name']}' parameter on {p.device}")
                if p.dim() < 1 or p.shape[0] != visibility.numel():
                    raise ValueError(f"the '{group['name']}' parameter has shape {tuple(p.shape)}, visibility has {visibility.numel()} rows")
                if not p.is_contiguous():
                    raise ValueError(f"the '{group['name']}' parameter is not row-major contiguous: its rows cannot be masked")


def _dense(t):
    """True when the tensor's elements tile one contiguous memory range in some dimension order (contiguous, channels_last,
    any permutation of a contiguous tensor): the kernel walks memory linearly, the logical order is irrelevant to Adam."""
    sizes_strides = sorted((st, sz) for sz, st in zip(t.shape, t.stride()) if sz > 1)
    expect = 1
    for st, sz in sizes_strides:
        if st != expect:
            return False
        expect *= sz
    return True
