"""LoRA injection with peft's surface (``peft.LoraConfig`` / ``peft.get_peft_model``), as used by the reference at
videotuna/models/cogvideo_hf/cogvideo_pl.py:143-149 with configs/004_cogvideox/cogvideo2b.yaml:32-38
(r=4, lora_alpha=1.0, target_modules to_k,to_q,to_v,to_out.0, init_lora_weights=True):

    y = W x + b + (lora_alpha / r) * B(A(x)),   A ~ kaiming_uniform(a=sqrt 5),  B = 0,  base frozen.

State-dict keys follow peft 0.12: ``base_model.model.<path>.base_layer.weight``,
``base_model.model.<path>.lora_A.default.weight`` -- the reference only relies on the substring "lora"
(cogvideo_pl.py:781-787, videotuna/utils/callbacks.py:44-46).  ``use_dora=True`` adds one fp32 magnitude per adapted Linear,
``base_model.model.<path>.lora_magnitude_vector.default.weight`` [out_features] (peft 0.12's DoraLinearLayer; the key is written from
memory of that release, peft is not a dependency), which the same substring rule saves and loads.

``target_modules`` may name any of the six Linears of a block (TARGETS: the attention projections and the feed-forward pair
ff.net.0.proj / ff.net.2), matched by peft's rule: a module is wrapped when its path equals a target or ends in "." + target.

All adapter weights live in ONE flat fp32 master buffer (plus a flat fp32 gradient buffer and a flat bf16 compute
copy) so the optimizer is one fused kernel launch and data-parallel training needs one all-reduce.
"""
from __future__ import annotations

import math
import os
import re
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import torch
import torch.nn as nn

TARGETS = ("to_q", "to_k", "to_v", "to_out.0", "ff.net.0.proj", "ff.net.2")
N_ATTN = 4             # TARGETS[:4]: the attention projections (adapter index j = 0..3); j = 4, 5: the feed-forward pair
# module paths of the CogVideoX DiT (dit.py), for peft's target rule on a model that is not an nn.Module: the adaptable Linears of a
# block (TARGETS order) and everything else a target could name
_BLOCK_LINEARS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "ff.net.0.proj", "ff.net.2")
_OTHER_PATHS = ("patch_embed", "patch_embed.proj", "patch_embed.text_proj", "time_embedding", "time_embedding.linear_1",
                "time_embedding.linear_2", "norm_final", "norm_out", "norm_out.linear", "norm_out.norm", "proj_out",
                "transformer_blocks", "transformer_blocks.0", "transformer_blocks.0.norm1", "transformer_blocks.0.norm1.linear",
                "transformer_blocks.0.norm1.norm", "transformer_blocks.0.norm2", "transformer_blocks.0.norm2.linear",
                "transformer_blocks.0.norm2.norm", "transformer_blocks.0.attn1", "transformer_blocks.0.attn1.norm_q",
                "transformer_blocks.0.attn1.norm_k", "transformer_blocks.0.attn1.to_out", "transformer_blocks.0.attn1.to_out.1",
                "transformer_blocks.0.ff", "transformer_blocks.0.ff.net", "transformer_blocks.0.ff.net.0", "transformer_blocks.0.ff.net.1")
_BLOCK_PATH = re.compile(r"transformer_blocks\.\d+\.(.+)$")


def resolve_targets(model, target_modules) -> List[str]:
    """The members of TARGETS that ``target_modules`` names by peft's rule -- a module is wrapped when its path equals a target or
    ends in "." + target -- in TARGETS order.  A target that matches nothing, or anything but the six block Linears (bare "proj"
    also matches patch_embed.proj, a convolution), raises."""
    if hasattr(model, "named_modules"):
        paths = [n for n, _ in model.named_modules() if n]
    else:
        paths = list(_OTHER_PATHS) + ["transformer_blocks.0." + b for b in _BLOCK_LINEARS]
    hit = set()
    for t in target_modules:
        matched = [p for p in paths if p == t or p.endswith("." + t)]
        subs = [_BLOCK_PATH.match(p) for p in matched]
        if not matched or any(m is None or m.group(1) not in _BLOCK_LINEARS for m in subs):
            raise ValueError(f"unsupported LoRA target {t!r}; the block Linears {TARGETS} of the CogVideoX DiT are supported")
        hit.update(_BLOCK_LINEARS.index(m.group(1)) for m in subs)
    return [TARGETS[j] for j in sorted(hit)]
NARROW_MAX_R = 16      # up to here the adapters ride in a fixed 64-column K-extension (csrc/lora.hip)
MAX_R = 128            # above NARROW_MAX_R: the wide layout on the MFMA rank-side kernels (csrc/lora_wide.hip)


def _ceil_to(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def extension_layout(r: int, wide: bool = None):
    """(rp, ext_qkv, ext_o, wide) of the K-extension for rank r: adapter j of a fused projection owns the extension columns
    [j*rp, j*rp + r).  r <= 16: rp = r inside a fixed 64-column extension; above (or for any rank with VT355_LORA_WIDE=1, a
    test / A-B knob): rp = r rounded up to a multiple of 16, so that every adapter's column block starts 16-byte aligned, and
    the extensions are 3 rp / rp columns rounded up to the GEMMs' 64-deep K step."""
    if wide is None:
        wide = r > NARROW_MAX_R or os.environ.get("VT355_LORA_WIDE", "0") not in ("", "0")
    if not wide:
        return r, 64, 64, False
    rp = _ceil_to(r, 16)
    return rp, _ceil_to(3 * rp, 64), _ceil_to(rp, 64), True


@dataclass
class LoraConfig:
    """peft.LoraConfig's fields as the CogVideoX recipes set them.  ``lora_dropout`` = p > 0: in training mode every adapted Linear
    drops elements of its own input before lora_A, ``(alpha/r) B A (keep * x) / (1 - p)`` with one mask per adapted Linear and forward,
    as peft's per-layer nn.Dropout does; model.eval() and p = 0 run the undropped kernels.  The masks come from Philox4x32-10 keyed by
    ``model.lora_dropout_seed`` (None: a fresh seed per forward from torch's CPU generator; the seed used is kept in
    ``model.last_lora_dropout_seed``), not from torch's device generator: statistically, not bit-wise, peft's masks."""
    r: int = 8
    lora_alpha: float = 8
    target_modules: Optional[Sequence[str]] = None
    lora_dropout: float = 0.0
    init_lora_weights: bool = True
    bias: str = "none"
    task_type: Optional[str] = None
    use_dora: bool = False           # weight-decomposed adapters: one trained magnitude per output feature (LoraState, DESIGN 3 "DoRA")
    use_rslora: bool = False         # scaling = lora_alpha / sqrt(r) instead of lora_alpha / r
    extra: dict = field(default_factory=dict)

    def __post_init__(self):
        if self.use_dora and float(self.lora_dropout) > 0.0:
            raise NotImplementedError("use_dora with lora_dropout > 0 is not supported: peft drops the input of the (c - 1) W x term as well, "
                                      "and a dropped base product cannot ride in the extended [W | s B] operand that DoRA scales")
        if not 0.0 <= float(self.lora_dropout) < 1.0:
            raise ValueError(f"lora_dropout must be in [0, 1), got {self.lora_dropout}")
        if self.bias != "none":
            raise NotImplementedError("bias != 'none' is not supported")
        if self.r <= 0 or self.r > MAX_R:
            raise NotImplementedError(f"rank 1..{MAX_R} per adapter: the rank-side kernels hold at most 3 adapters x {MAX_R} rank columns "
                                      f"of the K-extension; peft itself takes any rank")


class _W(nn.Module):
    """holder whose only parameter is ``weight`` (so keys read ``lora_A.default.weight``)."""

    def __init__(self, p: nn.Parameter):
        super().__init__()
        self.weight = p


class LoraLinear(nn.Module):
    def __init__(self, base: nn.Module, a: nn.Parameter, b: nn.Parameter, scaling: float, m: Optional[nn.Parameter] = None):
        super().__init__()
        self.base_layer = base
        self.lora_A = nn.ModuleDict({"default": _W(a)})
        self.lora_B = nn.ModuleDict({"default": _W(b)})
        if m is not None:          # use_dora: peft 0.12's DoraLinearLayer holds the magnitude as ``weight`` [out_features]
            self.lora_magnitude_vector = nn.ModuleDict({"default": _W(m)})
        self.scaling = {"default": scaling}
        self.in_features, self.out_features = base.in_features, base.out_features

    @property
    def weight(self):
        return self.base_layer.weight

    @property
    def bias(self):
        return self.base_layer.bias


class LoraState:
    """Flat storage for every adapter of a DiT.  Per layer: A_qkv [3r,d] | A_o [r,d] | B_qkv [3d,r] | B_o [d,r]; behind the L attention
    slabs, only when a feed-forward Linear is targeted, per layer: A_ff1 [r,d] | B_ff1 [4d,r] (ff.net.0.proj) and / or A_ff2 [r,4d] |
    B_ff2 [d,r] (ff.net.2) -- the attention part of the buffers is the same with and without them.  use_dora: behind all of these, per
    layer, the fp32 magnitudes m_q | m_k | m_v | m_o [4d] | m_ff1 [4d] | m_ff2 [d] (the feed-forward ones only when targeted), kind "M" of
    view(): the offsets of every A and B are the ones of a state without DoRA."""

    def __init__(self, model, cfg: LoraConfig):
        self.cfg = cfg
        self.r = cfg.r
        # K-extension layout: per-adapter column stride and the extension widths of the fused qkv / out operands
        self.rp, self.ext_qkv, self.ext_o, self.wide = extension_layout(cfg.r)
        self.scaling = float(cfg.lora_alpha) / (math.sqrt(cfg.r) if cfg.use_rslora else cfg.r)
        self.dora = bool(cfg.use_dora)
        self.p = float(cfg.lora_dropout)      # lora_dropout: > 0 selects the _drop rank-side kernels in training mode
        self.d = model.inner_dim
        self.L = model.config.num_layers
        self.targets = resolve_targets(model, list(cfg.target_modules or TARGETS[:N_ATTN]))
        self.ff1, self.ff2 = "ff.net.0.proj" in self.targets, "ff.net.2" in self.targets
        r, d = self.r, self.d
        self.per_layer = 8 * r * d
        # feed-forward adapters: one per Linear, so the K-extension is the single-adapter width of to_out.0
        self.dff = (int(getattr(model.config, "ff_mult", 4)) * d) if (self.ff1 or self.ff2) else 0
        self.ext_ff = self.ext_o
        self.ff_base = self.L * self.per_layer
        self.ff_off = {4: 0, 5: r * (d + self.dff) if self.ff1 else 0}         # offsets inside one layer's feed-forward slab
        self.ff_per_layer = r * (d + self.dff) * (int(self.ff1) + int(self.ff2))
        self.numel = self.L * (self.per_layer + self.ff_per_layer)
        # use_dora: the magnitudes follow every A / B slab (FusedAdamW and the data-parallel all-reduce see one longer buffer)
        self.mag_base = self.numel
        self.mag_off = {4: 4 * d, 5: 4 * d + (self.dff if self.ff1 else 0)}
        self.mag_per_layer = (4 * d + (self.dff if self.ff1 else 0) + (d if self.ff2 else 0)) if self.dora else 0
        self.numel += self.L * self.mag_per_layer
        dev = model.device
        self.flat = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        self.grad = torch.zeros_like(self.flat)
        self.flat_bf16 = torch.zeros(self.numel, dtype=torch.bfloat16, device=dev)
        self.version = 0              # bumped whenever the master weights change (optimizer step / load)
        self.params: List[nn.Parameter] = []

    # offsets inside one layer's slab
    def off_A(self, j):       # j: 0..2 = q,k,v ; 3 = out
        return j * self.r * self.d
    def off_B(self, j):
        return 4 * self.r * self.d + j * self.d * self.r

    def ff_dims(self, j):     # (in_features, out_features) of feed-forward Linear j: 4 = ff.net.0.proj, 5 = ff.net.2
        return (self.d, self.dff) if j == 4 else (self.dff, self.d)

    def mag_out(self, j):     # out_features of Linear j
        return self.d if j < N_ATTN else self.ff_dims(j)[1]

    def view(self, buf, layer, kind, j):
        if kind == "M":        # the magnitude of Linear j; j = 0..3 are adjacent: view(buf, layer, "M", 0)'s first 3d are the fused qkv's
            o = self.mag_base + layer * self.mag_per_layer + (j * self.d if j < N_ATTN else self.mag_off[j])
            return buf[o:o + self.mag_out(j)]
        if j >= N_ATTN:
            fin, fout = self.ff_dims(j)
            o = self.ff_base + layer * self.ff_per_layer + self.ff_off[j] + (0 if kind == "A" else self.r * fin)
            return buf[o:o + self.r * (fin if kind == "A" else fout)].view((self.r, fin) if kind == "A" else (fout, self.r))
        o = layer * self.per_layer + (self.off_A(j) if kind == "A" else self.off_B(j))
        n = self.r * self.d
        return buf[o:o + n].view((self.r, self.d) if kind == "A" else (self.d, self.r))

    def a_qkv(self, buf, layer):      # [3r, d] contiguous (q,k,v adapters stacked)
        o = layer * self.per_layer
        return buf[o:o + 3 * self.r * self.d].view(3 * self.r, self.d)

    def a_out(self, buf, layer):
        o = layer * self.per_layer + 3 * self.r * self.d
        return buf[o:o + self.r * self.d].view(self.r, self.d)

    def b_qkv(self, buf, layer):      # [3d, r]
        o = layer * self.per_layer + 4 * self.r * self.d
        return buf[o:o + 3 * self.d * self.r].view(3 * self.d, self.r)

    def b_out(self, buf, layer):
        o = layer * self.per_layer + 7 * self.r * self.d
        return buf[o:o + self.d * self.r].view(self.d, self.r)

    def mag_qkv(self, buf, layer):    # [3d]: the magnitudes of to_q | to_k | to_v (use_dora)
        o = self.mag_base + layer * self.mag_per_layer
        return buf[o:o + 3 * self.d]

    def init(self, seed: int = 1):
        g = torch.Generator().manual_seed(seed)
        bound = 1.0 / math.sqrt(self.d)
        host = torch.zeros(self.numel, dtype=torch.float32)
        for layer in range(self.L):
            for j, t in enumerate(TARGETS[:N_ATTN]):
                if t in self.targets:
                    a = (torch.rand((self.r, self.d), generator=g) * 2 - 1) * bound
                    o = layer * self.per_layer + self.off_A(j)
                    host[o:o + a.numel()] = a.reshape(-1)
        # the feed-forward adapters draw after every attention adapter (a seed's attention init does not depend on the target list),
        # each with peft's bound for its own in_features
        for layer in range(self.L):
            for j in range(N_ATTN, len(TARGETS)):
                if TARGETS[j] in self.targets:
                    fin = self.ff_dims(j)[0]
                    a = (torch.rand((self.r, fin), generator=g) * 2 - 1) / math.sqrt(fin)
                    self.view(host, layer, "A", j).copy_(a)
        with torch.no_grad():
            self.flat.copy_(host.to(self.flat.device))
        self.mark_changed()

    def init_magnitudes(self, model):
        """peft's dora_init: m = ||W + s B A|| row by row.  On the device the norms come from the kernel that computes them in every later
        refresh (ops.dora_norm), so c = m / norm is exactly 1.0f until an adapter or a magnitude changes; on a CPU model torch's fp32 norm."""
        from . import ops
        from .engine import _lin
        with torch.no_grad():
            if self.flat.is_cuda:
                ops.cast_f32_bf16(self.flat, self.flat_bf16)
            for layer, blk in enumerate(model.transformer_blocks):
                a = blk.attn1
                lins = (a.to_q, a.to_k, a.to_v, a.to_out[0], blk.ff.net[0].proj, blk.ff.net[2])
                for j, t in enumerate(TARGETS):
                    if t not in self.targets:
                        continue
                    w, m = _lin(lins[j])[0], self.view(self.flat, layer, "M", j)
                    if self.flat.is_cuda:
                        ops.dora_norm(w, self.view(self.flat_bf16, layer, "A", j), self.view(self.flat_bf16, layer, "B", j), 1, self.r,
                                      self.scaling, m)
                    else:
                        A, Bm = self.view(self.flat, layer, "A", j), self.view(self.flat, layer, "B", j)
                        m.copy_(torch.linalg.norm(w.float() + self.scaling * (Bm @ A), dim=1))
        self.mark_changed()

    def mark_changed(self):
        from . import ops
        if self.flat.is_cuda:
            ops.cast_f32_bf16(self.flat, self.flat_bf16)
        self.version += 1

    def attach_grads(self):
        """Point every adapter Parameter's .grad at its slice of the flat gradient buffer."""
        for p, (layer, kind, j) in zip(self.params, self._index):
            p.grad = self.view(self.grad, layer, kind, j)

    def dora_scratch(self, n: int):
        """a zeroed fp32 [n] scratch on the state's device (the backward pass: the unscaled dB products and the column sums of dm)"""
        buf = getattr(self, "_scratch", None)
        if buf is None or buf.numel() < n or buf.device != self.flat.device:
            buf = self._scratch = torch.empty(n, dtype=torch.float32, device=self.flat.device)
        return buf[:n].zero_()

    def on_module_moved(self):
        # nn.Module._apply moved / converted the Parameters individually: re-home them into one flat buffer
        if not self.params:
            return
        dev = self.params[0].device
        new_flat = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        for p, (layer, kind, j) in zip(self.params, self._index):
            self.view(new_flat, layer, kind, j).copy_(p.detach().to(torch.float32))
        self.flat = new_flat
        self.grad = torch.zeros_like(new_flat)
        self.flat_bf16 = torch.zeros(new_flat.numel(), dtype=torch.bfloat16, device=dev)
        for p, (layer, kind, j) in zip(self.params, self._index):
            p.data = self.view(self.flat, layer, kind, j)
        self.attach_grads()
        self.mark_changed()


def inject(model, cfg: LoraConfig, seed: int = 1) -> LoraState:
    """Freeze the base model and wrap the targeted projections (in place)."""
    st = LoraState(model, cfg)
    st._index = []
    for layer, blk in enumerate(model.transformer_blocks):
        for j, t in enumerate(TARGETS):
            if t not in st.targets:
                continue
            a = nn.Parameter(st.view(st.flat, layer, "A", j), requires_grad=True)
            b = nn.Parameter(st.view(st.flat, layer, "B", j), requires_grad=True)
            m = nn.Parameter(st.view(st.flat, layer, "M", j), requires_grad=True) if st.dora else None
            if t == "to_out.0":
                base = blk.attn1.to_out[0]
                blk.attn1.to_out[0] = LoraLinear(base, a, b, st.scaling, m)
            elif t == "ff.net.0.proj":
                blk.ff.net[0].proj = LoraLinear(blk.ff.net[0].proj, a, b, st.scaling, m)
            elif t == "ff.net.2":
                blk.ff.net[2] = LoraLinear(blk.ff.net[2], a, b, st.scaling, m)
            else:
                base = getattr(blk.attn1, t)
                setattr(blk.attn1, t, LoraLinear(base, a, b, st.scaling, m))
            st.params += [a, b]
            st._index += [(layer, "A", j), (layer, "B", j)]
            if st.dora:
                st.params.append(m)
                st._index.append((layer, "M", j))
    model.lora = st
    if cfg.init_lora_weights:
        st.init(seed)
    if st.dora:
        st.init_magnitudes(model)
    st.attach_grads()
    return st


class _LoraModel(nn.Module):       # peft's ``base_model`` level
    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, *a, **k):
        return self.model(*a, **k)

    def __getattr__(self, name):        # peft's BaseTuner forwards unknown attributes to the wrapped model as well
        try:
            return super().__getattr__(name)
        except AttributeError:
            if name == "model":
                raise
            return getattr(self.model, name)


class PeftModel(nn.Module):
    """Minimal stand-in for peft.PeftModel: same key prefix (``base_model.model.``) and attribute pass-through."""

    def __init__(self, model, cfg: LoraConfig):
        super().__init__()
        model.requires_grad_(False)
        self.peft_config = {"default": cfg}
        state = inject(model, cfg)
        self.base_model = _LoraModel(model)
        self._lora_state = state

    def forward(self, *a, **k):
        return self.base_model(*a, **k)

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            return getattr(self.base_model.model, name)

    def get_nb_trainable_parameters(self):
        tr = sum(p.numel() for p in self.parameters() if p.requires_grad)
        al = sum(p.numel() for p in self.parameters())
        return tr, al

    def print_trainable_parameters(self):
        tr, al = self.get_nb_trainable_parameters()
        print(f"trainable params: {tr:,d} || all params: {al:,d} || trainable%: {100 * tr / al:.4f}")


def get_peft_model(model, peft_config: LoraConfig) -> PeftModel:
    return PeftModel(model, peft_config)
