"""Fused AdamW (torch.optim.AdamW semantics and defaults: betas (0.9, 0.999), eps 1e-8, weight_decay 1e-2,
decoupled decay) -- what ``configure_optimizers`` returns in the reference (cogvideo_pl.py:774-779).

When the parameters are the adapter views of one ``LoraState`` the whole update is ONE kernel over the flat fp32
master buffer (which also refreshes the flat bf16 compute copy); otherwise one launch per tensor.

``gradient_clip_val`` / ``gradient_clip_algorithm`` are Lightning's trainer options.  'norm' is torch.nn.utils.clip_grad_norm_ over
all parameters of the optimizer, on the device: one read-only pass per gradient buffer for the squared norm (ops.grad_sqnorm), one
small launch that leaves ``{total_norm, clip_coef}`` in device memory (ops.clip_finalize), and an AdamW launch that multiplies each
gradient by that device word.  The gradient buffer is never rewritten and nothing is copied to the host.  'value' is
clip_grad_value_, a clamp inside the AdamW launch.  Under DDP call ``step`` only after the reducer's ``reduce()`` / ``wait()``:
the norm of the SUMMED gradient times ``grad_scale = 1 / world`` is the norm of the mean gradient, the same on every rank.
"""
from __future__ import annotations

from typing import Iterable, Optional

import torch

from . import ops


class FusedAdamW:
    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, lora_state=None, fullft_state=None, gradient_clip_val: Optional[float] = None,
                 gradient_clip_algorithm: str = "norm"):
        if gradient_clip_algorithm not in ("norm", "value"):
            raise ValueError(f"gradient_clip_algorithm {gradient_clip_algorithm!r}: 'norm' or 'value'")
        if gradient_clip_val is not None and not float(gradient_clip_val) >= 0.0:
            raise ValueError(f"gradient_clip_val {gradient_clip_val!r}: None / 0 (off) or a positive number")
        self.params = [p for p in params]
        if not self.params:
            raise ValueError("optimizer got an empty parameter list")
        if fullft_state is None:
            for p in self.params:
                if p.dtype != torch.float32:
                    raise TypeError("FusedAdamW keeps fp32 master weights; got a parameter of dtype %s "
                                    "(bf16 base weights need vt355.fullft.enable_full_finetune)" % p.dtype)
        self.defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, gradient_clip_val=gradient_clip_val,
                             gradient_clip_algorithm=gradient_clip_algorithm)
        self._clip_partials = self._clip_record = None      # device buffers of the norm pass, allocated at the first clipped step
        self.param_groups = [dict(params=self.params, **self.defaults)]
        self.lora_state = lora_state if lora_state is not None else fullft_state      # both expose flat / grad / flat_bf16 / version
        self.is_fullft = fullft_state is not None
        lora_state = self.lora_state
        self.step_count = 0
        self._err_host = self._err_event = None
        if self.is_fullft:
            self.m = torch.zeros_like(fullft_state.flat)
            self.v = torch.zeros_like(fullft_state.flat)
        elif lora_state is not None:
            if sum(p.numel() for p in self.params) != sum(p.numel() for p in lora_state.params):
                raise ValueError("flat mode needs exactly the adapter parameters of the LoraState")
            self.m = torch.zeros_like(lora_state.flat)
            self.v = torch.zeros_like(lora_state.flat)
        else:
            self.m = [torch.zeros_like(p) for p in self.params]
            self.v = [torch.zeros_like(p) for p in self.params]

    def zero_grad(self, set_to_none: bool = False):
        if self.lora_state is not None:
            self.lora_state.grad.zero_()
        else:
            for p in self.params:
                if p.grad is not None:
                    p.grad.zero_()

    def check_errors(self, wait: bool = True):
        """Raise if a kernel of an EARLIER step flagged its gradients invalid (a timed-out dQ hand-off of the attention
        backward: that step's update was refused on the device by vt_adamw's guard).  The flag travels to a pinned host
        word by an async copy queued behind each step; by the next step it has long arrived, so this does not stall."""
        if self._err_event is None:
            return
        if not wait and not self._err_event.query():
            return
        self._err_event.synchronize()
        self._err_event = None
        n = int(self._err_host.item())
        if n:
            from ._lib import VtError
            raise VtError(f"{n} dQ hand-off wait(s) of the attention backward timed out (persistent workgroups were not co-resident): "
                          "the gradients of that step were invalid and its optimizer update was skipped on the device. "
                          "Under DDP the word is shared (ddp.sync_chain_guard): every rank skipped together.  To go on: "
                          "vt355.ops.attn_bwd_chain_errors_clear() (the update of that step is lost), and declare concurrent streams with "
                          "vt355.ops.declare_side_stream(True) or set VT_BWD_CHAIN=1 so that it does not recur.")

    # ---- gradient clipping (settings live in param_groups[0], like lr) ----
    @property
    def gradient_clip_val(self):
        return self.param_groups[0].get("gradient_clip_val")

    @property
    def gradient_clip_algorithm(self):
        return self.param_groups[0].get("gradient_clip_algorithm", "norm")

    def _clip_mode(self):
        """None (off), 'norm' or 'value'"""
        return self.gradient_clip_algorithm if (self.gradient_clip_val or 0.0) > 0.0 else None

    @property
    def grad_norm(self):
        """0-dim DEVICE tensor: the global L2 norm of the gradient (times grad_scale) that the last clipped step measured, before
        clipping (what Lightning logs as grad_2.0_norm_total).  None unless gradient_clip_algorithm 'norm' is on; reading it with
        .item() synchronises and is the caller's choice."""
        return None if self._clip_mode() != "norm" else self._clip_buffers()[1][0]

    def _grad_buffers(self):
        if self.lora_state is not None:
            return [self.lora_state.grad]
        return [p.grad for p in self.params if p.grad is not None]

    def _clip_buffers(self, nslots: int = 1):
        dev = self.params[0].device
        if self._clip_record is None:
            self._clip_record = torch.zeros(2, dtype=torch.float32, device=dev)
        n = nslots * ops.grad_sqnorm_partials()
        if self._clip_partials is None or self._clip_partials.numel() < n:
            self._clip_partials = torch.empty(n, dtype=torch.float32, device=dev)
        return self._clip_partials, self._clip_record

    def _norm_pass(self, partials, slot: int) -> int:
        """squared-norm partials of every gradient buffer of this optimizer into consecutive slots from ``slot``; returns the next free slot"""
        for gbuf in self._grad_buffers():
            ops.grad_sqnorm(gbuf.view(-1), partials, slot)
            slot += 1
        return slot

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0, clip_coef: Optional[torch.Tensor] = None):
        """clip_coef: a device clip coefficient that the caller already computed over a wider set of parameters (the joint optimizer
        of a flow with several trained modules); otherwise, with 'norm' clipping on, it is computed here over this optimizer's own"""
        loss = closure() if closure is not None else None
        self.check_errors()
        self.step_count += 1
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        dev = self.params[0].device
        guard = ops.chain_guard(dev) if dev.type == "cuda" else None
        mode = self._clip_mode()
        clip = {}                       # off: the ops.adamw call of an optimizer built without the option, argument for argument
        if mode == "value":
            clip = dict(clip_value=float(g["gradient_clip_val"]))
        elif mode == "norm":
            if clip_coef is None:
                bufs = self._grad_buffers()
                if bufs:
                    partials, record = self._clip_buffers(len(bufs))
                    ops.clip_finalize(partials, self._norm_pass(partials, 0), grad_scale, float(g["gradient_clip_val"]), record)
                    clip_coef = record[1:2]
            clip = dict(clip_coef=clip_coef)
        elif clip_coef is not None:
            raise ValueError("clip_coef given to an optimizer whose gradient clipping is off")
        if self.lora_state is not None:
            st = self.lora_state
            ops.adamw(st.flat, st.grad, self.m, self.v, st.flat_bf16, g["lr"], b1, b2, g["eps"], g["weight_decay"],
                      self.step_count, grad_scale, guard, **clip)
            st.version += 1            # packed K-extension columns are refreshed at the next forward
        else:
            for p, m, v in zip(self.params, self.m, self.v):
                if p.grad is None:
                    continue
                ops.adamw(p.data, p.grad, m, v, None, g["lr"], b1, b2, g["eps"], g["weight_decay"], self.step_count,
                          grad_scale, guard, **clip)
        if guard is not None:
            if self._err_host is None:
                self._err_host = torch.zeros(1, dtype=torch.int32).pin_memory()
            self._err_host.copy_(guard, non_blocking=True)
            self._err_event = torch.cuda.Event()
            self._err_event.record(torch.cuda.current_stream(dev))
        return loss

    def state_dict(self):
        return dict(step=self.step_count, param_groups=[{k: v for k, v in g.items() if k != "params"} for g in self.param_groups],
                    m=self.m if torch.is_tensor(self.m) else list(self.m), v=self.v if torch.is_tensor(self.v) else list(self.v))

    def load_state_dict(self, sd):
        self.step_count = int(sd["step"])
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g.update(s)
        if torch.is_tensor(self.m):
            self.m.copy_(sd["m"]); self.v.copy_(sd["v"])
        else:
            for a, b in zip(self.m, sd["m"]):
                a.copy_(b)
            for a, b in zip(self.v, sd["v"]):
                a.copy_(b)
