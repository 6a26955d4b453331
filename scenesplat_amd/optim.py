"""FusedAdamW: gradient clipping + AdamW update of a whole model in three HIP launches (csrc/optim.hip).

torch.nn.utils.clip_grad_norm_ followed by torch.optim.AdamW.step walks the parameter memory about ten times per step in
separate multi-tensor launches and builds a parameter-sized temporary for the denominator.  Here the gradients are read once
for the global norm (two launches, the clip coefficient stays on the device) and one launch over the tensors of ALL parameter
groups reads p, g, m, v and writes p, m, v: 32 bytes per parameter.  Nothing is read on the host.

Opt-in through the registry (`optimizer=dict(type="FusedAdamW", ...)`); torch.optim.AdamW stays the default under "AdamW"."""
import math

import torch

from . import native as nv


class FusedAdamW(torch.optim.AdamW):
    """torch.optim.AdamW's arguments plus `max_grad_norm` (None: no clipping; the Trainer fills it from cfg["clip_grad"]).

    State layout is torch's own (`step`, `exp_avg`, `exp_avg_sq`, created lazily), so a state_dict() of torch.optim.AdamW loads
    into FusedAdamW and back.  Learning rate, betas, eps and weight decay are read from the param groups afresh every step
    (OneCycleLR with cycle_momentum writes them).

    The one observable difference from clip_grad_norm_ + AdamW: `p.grad` is left untouched.  The clipped gradient g * coef is
    formed in registers by the update kernel and never materialised, so code that reads p.grad after step() sees the
    unclipped gradient.  `last_grad_norm` holds the total norm (what clip_grad_norm_ returns) as a 0-d device tensor.

    Only CUDA, fp32, contiguous parameters with dense gradients are supported; anything else raises RuntimeError (there is no
    CPU fallback).  amsgrad, maximize, capturable, differentiable, foreach=True and fused=True are rejected."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None, max_grad_norm=None):
        for name, val in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable),
                          ("differentiable", differentiable), ("foreach", foreach), ("fused", fused)):
            if val:
                raise ValueError(f"FusedAdamW does not support {name}={val!r}")
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                         foreach=False, capturable=False, differentiable=False, fused=False)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None
        self._record = None

    # max_grad_norm travels with the checkpoint beside torch's own keys; a torch.optim.AdamW state dict (without it) loads as well.
    # A value this optimizer already has (constructor argument, or cfg["clip_grad"] through the Trainer) wins over the
    # checkpoint's: a run resumed with a changed clip_grad clips at the new value.
    def state_dict(self):
        sd = super().state_dict()
        sd["max_grad_norm"] = self.max_grad_norm
        return sd

    def load_state_dict(self, state_dict):
        sd = dict(state_dict)
        if "max_grad_norm" in sd:
            mg = sd.pop("max_grad_norm")
            if self.max_grad_norm is None and mg is not None:
                self.max_grad_norm = float(mg)
        super().load_state_dict(sd)
        for g in self.param_groups:
            for name in ("amsgrad", "maximize", "capturable", "differentiable", "foreach", "fused"):
                if g.get(name):
                    raise ValueError(f"FusedAdamW does not support {name}={g[name]!r} (from the loaded param group)")
        for st in self.state.values():          # `step` is read on the host every step: keep it there (a fused / capturable
            s = st.get("step")                  # torch optimizer saves it on the device)
            if torch.is_tensor(s) and s.device.type != "cpu":
                st["step"] = s.detach().to("cpu", torch.float32)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # every parameter with a gradient across all groups, refused by index before anything is touched
        todo, index, dev = [], 0, None
        for group in self.param_groups:
            for p in group["params"]:
                i, index = index, index + 1
                g = p.grad
                if g is None:
                    continue
                if not p.is_cuda or not g.is_cuda:
                    raise RuntimeError(f"FusedAdamW: parameter {i} is not on a GPU (no CPU fallback)")
                if g.layout is not torch.strided:
                    raise RuntimeError(f"FusedAdamW: parameter {i} has a sparse gradient")
                if p.dtype is not torch.float32 or g.dtype is not torch.float32:
                    raise RuntimeError(f"FusedAdamW: parameter {i} is {p.dtype} with a {g.dtype} gradient, fp32 only")
                if not p.is_contiguous() or not g.is_contiguous():
                    raise RuntimeError(f"FusedAdamW: parameter {i} or its gradient is not contiguous")
                dev = p.device if dev is None else dev
                if p.device != dev or g.device != dev:
                    raise RuntimeError(f"FusedAdamW: parameter {i} lives on another device than the parameters before it")
                todo.append((group, p, g))
        if not todo:
            return loss
        record = None
        if self.max_grad_norm is not None:
            if self._record is None or self._record.device != dev:
                self._record = torch.empty(2, dtype=torch.float32, device=dev)
                self.last_grad_norm = self._record[0]
            record = nv.grad_norm_group([g for _, _, g in todo], self.max_grad_norm, self._record)
        # state as torch lays it out, created lazily; `step` lives on the host, so the scalars below need no device read
        states = []
        for _, p, _ in todo:
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            states.append(st)
        torch._foreach_add_([st["step"] for st in states], 1)
        # per-tensor scalars in double, as torch's single-tensor AdamW computes them (one tuple per (group, t) pair)
        rows, params, cache = [], [], {}
        for (group, p, g), st in zip(todo, states):
            t = float(st["step"])
            s = cache.get((id(group), t))
            if s is None:
                lr, wd, eps = float(group["lr"]), float(group["weight_decay"]), float(group["eps"])
                beta1, beta2 = (float(b) for b in group["betas"])
                s = cache[(id(group), t)] = (1.0 - lr * wd, 1.0 - beta1, beta2, 1.0 - beta2, math.sqrt(1.0 - beta2 ** t), eps,
                                             lr / (1.0 - beta1 ** t))
            rows.append((p, g, st["exp_avg"], st["exp_avg_sq"], s))
            params.append(p)
        nv.adamw_group(rows, record)
        # the kernel wrote through raw pointers: bump the version counters, which the bf16 shadows (functional._stamp) and
        # autograd's saved-tensor checks key on
        torch.autograd.graph.increment_version(params)
        return loss
