"""Flat-buffer AdamW: the whole model's update in one HIP kernel.

``torch.optim.AdamW(foreach=True)`` still issues ~10 launches over a
list of tensors; for the launch-bound captured train step
(train/captured.py) this optimizer flattens all fp32 parameters into
ONE contiguous buffer at construction (parameters become views), keeps
a matching flat gradient buffer that autograd accumulates into, and
steps with the single fused kernel (csrc/fused_adamw.hip).  On CPU it
applies the same fp32 formula with flat torch ops, so the trajectory is
testable against torch.optim.AdamW without a GPU.

Contract (docs/kernels.md, "Optimizer"):

- every constant (lr, betas, eps, 1-b1, 1-b2, 1-lr*wd, 1-b^t) is formed
  in double and rounded to fp32 once; one step then stays within the
  rounding-count bound derived in tests/_exact_adamw.py, on the device
  and in the fallback alike;
- in bf16 mode the fp32 master is authoritative only while it still
  rounds to the stored bf16 parameter; an element whose parameter was
  overwritten from outside (``load_state_dict``, a broadcast) restarts
  from the overwritten value;
- parameters and gradients must remain the views created here.
  ``step()`` compares pointers and shapes on the host and raises if one
  was replaced (``model.zero_grad()``, ``p.grad = None``,
  ``model.to(...)``): use this optimizer's ``zero_grad`` and construct
  after moving the model;
- one parameter group.

Construct BEFORE any DDP wrapping so reducer bucket views are built
over the flattened storages.

Role parity: the reference trains with stock torch.optim selected by
``utils/optimizer`` (reference hydragnn/utils/optimizer/optimizer.py);
this fused optimizer is the MI355X-native drop-in used by the
launch-bound captured path (select_optimizer still provides every
reference optimizer type).
"""

from __future__ import annotations

import torch

from ._extension import get_extension, use_eager


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3,
                 betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2):
        params = list(params)
        group = {}
        if params and isinstance(params[0], dict):
            if len(params) > 1:
                raise ValueError(
                    f"FusedAdamW steps one flat buffer with one set of "
                    f"hyperparameters: got {len(params)} parameter "
                    f"groups, pass a single group")
            group = {k: v for k, v in params[0].items() if k != "params"}
            params = params[0]["params"]
            params = [params] if isinstance(params, torch.Tensor) \
                else list(params)
        params = [p for p in params if p.requires_grad]
        if not params:
            raise ValueError("FusedAdamW: no parameters")
        dtypes = {p.dtype for p in params}
        if dtypes == {torch.float32}:
            self.param_dtype = torch.float32
        elif dtypes == {torch.bfloat16}:
            # pure-bf16 training: bf16 working params + fp32 master
            self.param_dtype = torch.bfloat16
        else:
            raise TypeError(
                "FusedAdamW supports uniform fp32 or bf16 parameters")
        defaults = dict(lr=lr, betas=betas, eps=eps,
                        weight_decay=weight_decay)
        self._single_group_built = False
        super().__init__([dict(group, params=params)], defaults)
        self._single_group_built = True

        device = params[0].device
        total = sum(p.numel() for p in params)
        self.flat_param = torch.empty(total, dtype=self.param_dtype,
                                      device=device)
        self.flat_grad = torch.zeros(total, dtype=self.param_dtype,
                                     device=device)
        self.exp_avg = torch.zeros(total, dtype=torch.float32,
                                   device=device)
        self.exp_avg_sq = torch.zeros(total, dtype=torch.float32,
                                      device=device)
        self.step_t = torch.zeros(1, dtype=torch.float32,
                                  device=device)
        # (1 - b1^t, 1 - b2^t) of the current step, written by the
        # kernel's prelude
        self.bias_corr = torch.ones(2, dtype=torch.float32,
                                    device=device)
        off = 0
        self._params = params
        self._views = []     # (data pointer, grad pointer) per parameter
        with torch.no_grad():
            for p in params:
                n = p.numel()
                self.flat_param[off:off + n].copy_(p.reshape(-1))
                p.data = self.flat_param[off:off + n].view_as(p)
                p.grad = self.flat_grad[off:off + n].view_as(p)
                self._views.append((p.data_ptr(), p.grad.data_ptr()))
                off += n
        self.master = (self.flat_param.float()
                       if self.param_dtype == torch.bfloat16 else None)

    def add_param_group(self, param_group):
        if getattr(self, "_single_group_built", False):
            raise ValueError(
                "FusedAdamW steps one flat buffer built at construction: "
                "a parameter group cannot be added afterwards; build a "
                "new optimizer over all parameters")
        super().add_param_group(param_group)

    def zero_grad(self, set_to_none: bool = True):
        # grads are views into the flat buffer: never drop them
        self.flat_grad.zero_()

    def _check_views(self):
        """Host-only: every p.data / p.grad is still the view into the
        flat buffers that __init__ created (pointers and shapes; the
        device is not read)."""
        for i, (p, (dptr, gptr)) in enumerate(zip(self._params,
                                                  self._views)):
            grad = p.grad
            if p.data_ptr() == dptr and grad is not None \
                    and grad.data_ptr() == gptr \
                    and grad.shape == p.shape:
                continue
            what = ("its data was replaced" if p.data_ptr() != dptr
                    else "its .grad was dropped" if grad is None
                    else "its .grad was replaced")
            raise RuntimeError(
                f"FusedAdamW: parameter {i} (shape {tuple(p.shape)}) is "
                f"no longer a view into the optimizer's flat buffers: "
                f"{what}, so this step would not train it.  Clear "
                f"gradients with the optimizer's zero_grad() (not "
                f"model.zero_grad() or p.grad = None), and construct "
                f"FusedAdamW after moving or casting the model.")

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self._check_views()
        g = self.param_groups[0]
        lr, (b1, b2) = float(g["lr"]), g["betas"]
        eps, wd = g["eps"], g["weight_decay"]
        if self.flat_param.is_cuda and not use_eager():
            ext = get_extension(required=True)
            if self.master is None:
                ext.fused_adamw(self.flat_param, self.flat_grad,
                                self.exp_avg, self.exp_avg_sq,
                                self.step_t, self.bias_corr,
                                lr, b1, b2, eps, wd)
            else:
                ext.fused_adamw_bf16(self.flat_param, self.flat_grad,
                                     self.master, self.exp_avg,
                                     self.exp_avg_sq, self.step_t,
                                     self.bias_corr,
                                     lr, b1, b2, eps, wd)
            return loss
        # CPU / eager fallback: the kernel's fp32 formula on the flat
        # buffers.  Python scalars are doubles that torch rounds to
        # fp32 once, like the kernel's constants.
        self.step_t += 1
        t = int(self.step_t.item())
        bc1 = 1.0 - b1 ** t
        bc2 = 1.0 - b2 ** t
        self.bias_corr[0] = bc1
        self.bias_corr[1] = bc2
        if self.master is not None:
            # master reconciliation, as in the kernel: where the master
            # no longer rounds to the stored parameter, the parameter
            # was overwritten and the step starts from it
            stale = self.master.bfloat16().view(torch.int16) \
                != self.flat_param.view(torch.int16)
            self.master.copy_(torch.where(stale, self.flat_param.float(),
                                          self.master))
            work, g32 = self.master, self.flat_grad.float()
        else:
            work, g32 = self.flat_param, self.flat_grad
        work.mul_(1.0 - lr * wd)
        self.exp_avg.mul_(b1).add_(g32, alpha=1.0 - b1)
        self.exp_avg_sq.mul_(b2).add_((g32 * (1.0 - b2)).mul_(g32))
        denom = (self.exp_avg_sq / bc2).sqrt_().add_(eps)
        work.sub_((self.exp_avg / bc1).mul_(lr).div_(denom))
        if self.master is not None:
            self.flat_param.copy_(work)
        return loss

    def state_dict(self):
        group = {k: v for k, v in self.param_groups[0].items()
                 if k != "params"}
        group["params"] = list(range(len(self._params)))
        return {
            "param_groups": [group],
            "flat": {"exp_avg": self.exp_avg,
                     "exp_avg_sq": self.exp_avg_sq,
                     "step": self.step_t,
                     "master": self.master},
        }

    def load_state_dict(self, sd):
        if not isinstance(sd, dict) or "flat" not in sd:
            raise ValueError(
                "FusedAdamW.load_state_dict: the state has no 'flat' "
                "section, so it was not saved by FusedAdamW (a "
                "torch.optim.AdamW checkpoint keeps per-parameter "
                "state and cannot be loaded here)")
        flat = sd["flat"]
        for name in ("exp_avg", "exp_avg_sq"):
            if flat[name].numel() != self.exp_avg.numel():
                raise ValueError(
                    f"FusedAdamW.load_state_dict: {name} holds "
                    f"{flat[name].numel()} elements, this optimizer "
                    f"{self.exp_avg.numel()}")
        if flat.get("master") is not None and self.master is not None:
            self.master.copy_(flat["master"])
        self.exp_avg.copy_(flat["exp_avg"])
        self.exp_avg_sq.copy_(flat["exp_avg_sq"])
        self.step_t.copy_(flat["step"])
        for g, gs in zip(self.param_groups, sd["param_groups"]):
            g.update({k: v for k, v in gs.items() if k != "params"})
