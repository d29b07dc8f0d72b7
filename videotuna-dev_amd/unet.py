"""VideoCrafter2 denoiser on the vt355 kernels: ``UNetModel`` with the constructor keys, parameter names and ``forward`` signature
of videotuna/models/lvdm/modules/networks/openaimodel3d.py:313-694 (so ``configs/001_videocrafter2/*.yaml``'s ``denoiser_config`` /
``unet_config`` node instantiates it through the target remap), and the forward / backward schedule of its blocks
(ResBlock + TemporalConvBlock :123-310, Down/Upsample :56-120, SpatialTransformer / TemporalTransformer / CrossAttention / GEGLU
lvdm/modules/attention.py:45-548) -- BASELINE configs[3], SURVEY 8(a) a11-a13.

MI355X-first layout: ONE channels-last activation layout [B, T, H, W, C] (rows = positions, bf16) from the first convolution to the
last.  The reference's ``(b t) c h w <-> b c t h w <-> (b h w) c t`` rearranges (openaimodel3d.py:45-47, 249-253; attention.py:476-516)
do not exist: a Conv2d is the implicit-GEMM kernel with one temporal tap, the (3,1,1) convolution the same kernel with one spatial
tap, GroupNorm over (b t) or over b is a choice of (N, P) on the same buffer, a Linear is a GEMM over the rows, spatial attention
reads [B*T, H*W] sequences in place and the temporal transformer needs one row transpose each way.  Convolution weights live in
channels-last memory format (logical torch shape, tap-major storage), so the kernels' operands are views of the flat parameter
buffer and their weight gradients land in the flat fp32 gradient buffer without repacking.

Training (full fine-tune, the configs' recipe): one autograd node for the whole network; the forward records a tape of closures,
the backward replays it in reverse and accumulates parameter gradients (``+=``) into ``model.train_state.grad``.  Activations are
kept (no per-block recompute: 288 GB of HBM; the reference checkpoints every block, ``use_checkpoint: true``).
Train mode (``model.train()``, the nn.Module default, with gradients enabled): TemporalConvBlock's three nn.Dropout(0.1)
(:278-296, hard-coded at :205-210) are applied -- ``vt_dropout_bf16``, a counter-based Philox mask that is a pure function of (seed,
site, element), so the backward pass re-derives it and nothing is stored; a fresh seed per forward comes from torch's CPU generator
(``torch.manual_seed`` reproduces a run), ``model.dropout_seed = s`` pins it.  ``model.eval()`` switches the masks off (the golden
fixtures of the reference were taken that way).
DynamiCrafter (configs/002_dynamicrafter, openaimodel3d_dc.py) is the same network with ``img_cross_attention`` (every spatial attn2
gets to_k_ip / to_v_ip and a second softmax over the 16 image tokens of the query's frame: csrc/attn_dual.hip), ``fs_condition``
(the fps_embedding path, fed by ``fs``), 8 input channels and ResBlock dropout; the gradient of the image context rows is returned
through autograd because the Resampler that produces them trains.
There is no CPU / eager fallback.
"""
from __future__ import annotations

import math
import os
from types import SimpleNamespace
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import ops
from .ops import BF16, EPI_BIAS, EPI_GATED_RES

F32 = torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# module tree: layer descriptors in the order of UNetModel.__init__ (openaimodel3d.py:341-648)
# ---------------------------------------------------------------------------------------------------------------------
def build_structure(c) -> SimpleNamespace:
    mc, hd = c.model_channels, c.num_head_channels
    L = lambda kind, pre, **kw: SimpleNamespace(kind=kind, pre=pre, **kw)
    inp = [[L("conv_in", "input_blocks.0.0", cin=c.in_channels, cout=mc)]]
    chans = [mc]
    ch, ds, idx = mc, 1, 1
    for level, mult in enumerate(c.channel_mult):
        for _ in range(c.num_res_blocks):
            layers = [L("res", f"input_blocks.{idx}.0", cin=ch, cout=mult * mc, tconv=c.temporal_conv)]
            ch = mult * mc
            if ds in c.attention_resolutions:
                layers.append(L("st", f"input_blocks.{idx}.1", c=ch, heads=ch // hd, inner=ch))
                if c.temporal_attention:
                    layers.append(L("tt", f"input_blocks.{idx}.2", c=ch, heads=ch // hd, inner=ch))
            inp.append(layers); chans.append(ch); idx += 1
        if level != len(c.channel_mult) - 1:
            inp.append([L("down", f"input_blocks.{idx}.0", c=ch)]); chans.append(ch); idx += 1
            ds *= 2
    init_attn = L("tt", "init_attn.0", c=mc, heads=8, inner=8 * hd, conv1d=True) if c.addition_attention else None
    mid = [L("res", "middle_block.0", cin=ch, cout=ch, tconv=c.temporal_conv), L("st", "middle_block.1", c=ch, heads=ch // hd, inner=ch)]
    if c.temporal_attention:
        mid.append(L("tt", "middle_block.2", c=ch, heads=ch // hd, inner=ch))
    mid.append(L("res", f"middle_block.{len(mid)}", cin=ch, cout=ch, tconv=c.temporal_conv))
    out, idx = [], 0
    for level, mult in list(enumerate(c.channel_mult))[::-1]:
        for i in range(c.num_res_blocks + 1):
            ich = chans.pop()
            layers = [L("res", f"output_blocks.{idx}.0", cin=ch + ich, cout=mult * mc, tconv=c.temporal_conv)]
            ch = mult * mc
            if ds in c.attention_resolutions:
                layers.append(L("st", f"output_blocks.{idx}.{len(layers)}", c=ch, heads=ch // hd, inner=ch))
                if c.temporal_attention:
                    layers.append(L("tt", f"output_blocks.{idx}.{len(layers)}", c=ch, heads=ch // hd, inner=ch))
            if level and i == c.num_res_blocks:
                layers.append(L("up", f"output_blocks.{idx}.{len(layers)}", c=ch))
                ds //= 2
            out.append(layers); idx += 1
    return SimpleNamespace(input=inp, init_attn=init_attn, middle=mid, output=out, out_ch=ch)


def _param_shapes(c, st) -> Dict[str, tuple]:
    """reference state_dict keys in registration order"""
    mc, te = c.model_channels, 4 * c.model_channels
    sh: Dict[str, tuple] = {}
    for n in ["time_embed"] + (["fps_embedding"] if (c.fps_cond or c.fs_condition) else []):
        sh[n + ".0.weight"] = (te, mc); sh[n + ".0.bias"] = (te,)
        sh[n + ".2.weight"] = (te, te); sh[n + ".2.bias"] = (te,)

    def transformer(l, ctx_dim, img=False, rel=False):
        pre, cc, inner = l.pre, l.c, l.inner
        k1 = (1,) if getattr(l, "conv1d", False) else ()
        sh[pre + ".norm.weight"] = (cc,); sh[pre + ".norm.bias"] = (cc,)
        sh[pre + ".proj_in.weight"] = (inner, cc) + k1; sh[pre + ".proj_in.bias"] = (inner,)
        b = pre + ".transformer_blocks.0."

        def attn(a, kd, ip=False):
            sh[b + a + ".to_q.weight"] = (inner, inner); sh[b + a + ".to_k.weight"] = (inner, kd); sh[b + a + ".to_v.weight"] = (inner, kd)
            sh[b + a + ".to_out.0.weight"] = (inner, inner); sh[b + a + ".to_out.0.bias"] = (inner,)
            if ip:          # CrossAttention(img_cross_attention=True) registers the image projections after to_out (attention.py:82-84)
                sh[b + a + ".to_k_ip.weight"] = (inner, kd); sh[b + a + ".to_v_ip.weight"] = (inner, kd)
            if rel:         # CrossAttention(relative_position=True): two RelativePosition tables shared by the heads (attention.py:19-42, 87-95)
                for t in ("relative_position_k", "relative_position_v"):
                    sh[b + a + "." + t + ".embeddings_table"] = (2 * c.temporal_length + 1, c.num_head_channels)
        attn("attn1", inner)
        sh[b + "ff.net.0.proj.weight"] = (8 * inner, inner); sh[b + "ff.net.0.proj.bias"] = (8 * inner,)
        sh[b + "ff.net.2.weight"] = (inner, 4 * inner); sh[b + "ff.net.2.bias"] = (inner,)
        attn("attn2", inner if ctx_dim is None else ctx_dim, img)
        for n in ("norm1", "norm2", "norm3"):
            sh[b + n + ".weight"] = (inner,); sh[b + n + ".bias"] = (inner,)
        sh[pre + ".proj_out.weight"] = (cc, inner) + k1; sh[pre + ".proj_out.bias"] = (cc,)

    def add(l):
        pre = l.pre
        if l.kind == "conv_in":
            sh[pre + ".weight"] = (l.cout, l.cin, 3, 3); sh[pre + ".bias"] = (l.cout,)
        elif l.kind == "res":
            ci, co = l.cin, l.cout
            sh[pre + ".in_layers.0.weight"] = (ci,); sh[pre + ".in_layers.0.bias"] = (ci,)
            sh[pre + ".in_layers.2.weight"] = (co, ci, 3, 3); sh[pre + ".in_layers.2.bias"] = (co,)
            sh[pre + ".emb_layers.1.weight"] = (co, te); sh[pre + ".emb_layers.1.bias"] = (co,)
            sh[pre + ".out_layers.0.weight"] = (co,); sh[pre + ".out_layers.0.bias"] = (co,)
            sh[pre + ".out_layers.3.weight"] = (co, co, 3, 3); sh[pre + ".out_layers.3.bias"] = (co,)
            if ci != co:
                sh[pre + ".skip_connection.weight"] = (co, ci, 1, 1); sh[pre + ".skip_connection.bias"] = (co,)
            if l.tconv:
                for j in (1, 2, 3, 4):
                    last = 2 if j == 1 else 3
                    sh[pre + f".temopral_conv.conv{j}.0.weight"] = (co,); sh[pre + f".temopral_conv.conv{j}.0.bias"] = (co,)
                    sh[pre + f".temopral_conv.conv{j}.{last}.weight"] = (co, co, 3, 1, 1)
                    sh[pre + f".temopral_conv.conv{j}.{last}.bias"] = (co,)
        elif l.kind == "st":
            transformer(l, c.context_dim, c.img_cross_attention)
        elif l.kind == "tt":
            transformer(l, None, rel=c.use_relative_position)
        elif l.kind == "down":
            sh[pre + ".op.weight"] = (l.c, l.c, 3, 3); sh[pre + ".op.bias"] = (l.c,)
        elif l.kind == "up":
            sh[pre + ".conv.weight"] = (l.c, l.c, 3, 3); sh[pre + ".conv.bias"] = (l.c,)

    for blk in st.input:
        for l in blk:
            add(l)
    if st.init_attn is not None:
        add(st.init_attn)
    for l in st.middle:
        add(l)
    for blk in st.output:
        for l in blk:
            add(l)
    sh["out.0.weight"] = (st.out_ch,); sh["out.0.bias"] = (st.out_ch,)
    sh["out.2.weight"] = (c.out_channels, mc, 3, 3); sh["out.2.bias"] = (c.out_channels,)
    return sh


class _Node(nn.Module):
    pass


def _is_conv(shape) -> bool:
    return len(shape) in (4, 5)


class FlatParamModule(nn.Module):
    """A module whose parameters (reference names and logical shapes, given as an ordered {name: shape} dict) are views of ONE flat bf16
    buffer -- convolution weights in channels-last storage --, with an optional training state next to it (fp32 master + fp32 gradient
    buffer, one fused AdamW launch).  Shared by the VideoCrafter2 UNet and the OpenSora STDiT."""

    def _setup_flat(self, shapes: Dict[str, tuple], root: Optional[nn.Module] = None):
        """root: register the nn.Parameters in ANOTHER module's tree (the adapters of a LoRA'd UNet live under the UNet's own module paths,
        as peft names them) while the flat buffers stay with this object"""
        self.shapes = shapes
        self.offsets: Dict[str, int] = {}
        off = 0
        for n, shp in self.shapes.items():
            self.offsets[n] = off
            off += (math.prod(shp) + 7) // 8 * 8            # every parameter starts on a 16-byte boundary of the flat buffer
        self.numel = off
        self.flat_bf16 = torch.zeros(off, dtype=BF16)
        self._plist: Dict[str, nn.Parameter] = {}
        for n, shp in self.shapes.items():
            p = nn.Parameter(self._view(self.flat_bf16, n), requires_grad=True)
            self._plist[n] = p
            node = self if root is None else root
            parts = n.split(".")
            for a in parts[:-1]:
                if not hasattr(node, a):
                    node.add_module(a, _Node())
                node = getattr(node, a)
            node.register_parameter(parts[-1], p)
        self.train_state = None
        self._packed = None
        self._packed_version = -1

    # ---- flat storage ----
    def _view(self, buf, name):
        shp = self.shapes[name]
        o = self.offsets[name]
        v = buf[o:o + math.prod(shp)]
        if len(shp) == 4:       # conv weight [Cout, Cin, KH, KW]: channels-last storage = the kernels' tap-major operand
            return v.view(shp[0], shp[2], shp[3], shp[1]).permute(0, 3, 1, 2)
        if len(shp) == 5:
            return v.view(shp[0], shp[2], shp[3], shp[4], shp[1]).permute(0, 4, 1, 2, 3)
        return v.view(shp)

    def flat(self, buf, name, rows=None):
        """2-d operand view of a parameter in a flat buffer: Linear [N, K]; conv [Cout, taps*Cin]; vector [n]"""
        shp = self.shapes[name]
        o = self.offsets[name]
        v = buf[o:o + math.prod(shp)]
        return v.view(shp[0], -1) if len(shp) > 1 else v

    def span(self, buf, first, last):
        """rows of `first` .. `last` (adjacent [*, K] matrices in the flat layout, e.g. to_q | to_k | to_v) as ONE [sum N, K] matrix"""
        o0 = self.offsets[first]
        o1 = self.offsets[last] + math.prod(self.shapes[last])
        K = self.shapes[first][1]
        return buf[o0:o1].view(-1, K)

    def _apply(self, fn, *a, **k):
        if self.train_state is not None:
            raise RuntimeError("move / convert the model BEFORE enable_training(): optimizer state lives next to the parameters")
        out = super()._apply(fn, *a, **k)
        self._reflat()
        return out

    def _reflat(self):
        """after a dtype / device change of the parameters: gather them into a fresh flat buffer and make them views of it again"""
        p0 = next(iter(self._plist.values()))
        new = torch.zeros(self.numel, dtype=p0.dtype, device=p0.device)
        for n, p in self._plist.items():
            self._view(new, n).copy_(p.detach())
            p.data = self._view(new, n)
        self.flat_bf16 = new
        self._packed = None

    def load_state_dict(self, sd, strict: bool = True, **kw):
        out = super().load_state_dict({k: (v.to(BF16) if k in self.shapes else v) for k, v in sd.items()}, strict=strict, **kw)
        if self.train_state is not None:
            self.train_state.flat.copy_(self.flat_bf16)
            self.train_state.version += 1
        self._packed = None
        return out

    def enable_training(self):
        """full fine-tuning state: fp32 master copy and fp32 gradient buffer next to the flat bf16 parameters; hand
        ``model.train_state`` to FusedAdamW(fullft_state=...)"""
        if getattr(self, "lora", None) is not None and not isinstance(self, _UNetLora):
            raise RuntimeError("this model carries LoRA adapters: its base weights are frozen, train with enable_lora_training()")
        if self.flat_bf16.dtype != BF16:
            raise TypeError("the MI355X engine computes in bf16: call .bfloat16() first")
        if self.train_state is None:
            ts = SimpleNamespace(flat=self.flat_bf16.to(F32), grad=torch.zeros(self.numel, dtype=F32, device=self.flat_bf16.device),
                                 flat_bf16=self.flat_bf16, params=list(self._plist.values()), version=0, numel=self.numel,
                                 on_grads_ready=None)
            ts.g = lambda name: self.flat(ts.grad, name)
            self.train_state = ts
        return self.train_state

    @property
    def dtype(self):
        return self.flat_bf16.dtype

    @property
    def device(self):
        return self.flat_bf16.device


EXT = 64          # K-extension columns of a LoRA'd Linear: x_ext = [x | x A^T (adapters x r <= 64 columns) | 0], W_ext = [W | scaling B | 0]
LORA_TARGETS = ("to_q", "to_k", "to_v")


class _UNetLora(FlatParamModule):
    """Rank-r adapters on the attention projections of every CrossAttention -- the modules peft's suffix match selects for the shipped recipe
    (configs/001_videocrafter2/vc2_t2v_lora.yaml:7-12: target_modules to_q / to_k / to_v, lora_rank 4, lora_alpha 1; injected by
    videotuna/models/lvdm/ddpm3d.py:100-117, 434-445).  Parameters carry peft's names inside the UNet's own module tree:
    ``<path>.to_q.lora_A.default.weight`` [r, in], ``<path>.to_q.lora_B.default.weight`` [out, r]; they are views of this object's flat
    buffer (one fp32 master / gradient buffer, one fused AdamW launch)"""

    def __init__(self, unet: "UNetModel", r: int, lora_alpha: float, target_modules):
        super().__init__()
        tm = tuple(target_modules)
        bad = [t for t in tm if t not in LORA_TARGETS]
        if bad:
            raise NotImplementedError(f"LoRA targets {bad}: the attention projections {LORA_TARGETS} are supported (the recipe's)")
        if r <= 0 or 3 * r > EXT:
            raise ValueError(f"rank {r}: three adapters must fit the {EXT} extension columns")
        self.r, self.scaling, self.targets = int(r), float(lora_alpha) / r, tm
        self.sites = [n[:-7] for n in unet.shapes if n.endswith(".weight") and any(n[:-7].endswith("." + t) for t in tm)]
        sh: Dict[str, tuple] = {}
        for mod in self.sites:
            out_f, in_f = unet.shapes[mod + ".weight"]
            sh[mod + ".lora_A.default.weight"] = (r, in_f)
            sh[mod + ".lora_B.default.weight"] = (out_f, r)
        self._setup_flat(sh, root=unet)
        self.shapes_sites = set(self.sites)

    def init_weights(self, seed: int = 0, zero_b: bool = True):
        """peft's default: A random, B zero (the adapter starts as the identity); zero_b=False for tests"""
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for n, p in self._plist.items():
                shp = self.shapes[n]
                if ".lora_A." in n:
                    w = torch.randn(shp, generator=g) * shp[1] ** -0.5
                else:
                    w = torch.zeros(shp) if zero_b else torch.randn(shp, generator=g) * 0.05
                p.copy_(w.to(p.device, BF16))
        self.weights_changed()
        return self

    def weights_changed(self):
        """the adapter tensors were written directly (checkpoint load): the fp32 master and the packed operands follow"""
        if self.train_state is not None:
            self.train_state.flat.copy_(self.flat_bf16)
            self.train_state.version += 1
        self._packed = None


class UNetModel(FlatParamModule):
    """Constructor keys of the reference's UNetModel (openaimodel3d.py:341-372); options the VideoCrafter2 recipes leave off are
    refused instead of ignored."""

    def __init__(self, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions, dropout=0.0,
                 channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, context_dim=None, use_scale_shift_norm=False,
                 resblock_updown=False, num_heads=-1, num_head_channels=-1, transformer_depth=1, use_linear=False, use_checkpoint=False,
                 temporal_conv=False, tempspatial_aware=False, temporal_attention=True, temporal_selfatt_only=True,
                 use_relative_position=True, use_causal_attention=False, temporal_length=None, use_fp16=False,
                 addition_attention=False, use_image_attention=False, temporal_transformer_depth=1, fps_cond=False,
                 text_context_len: int = 77, img_cross_attention=False, img_cross_attention_scale_learnable=False, default_fs=4,
                 fs_condition=False):
        super().__init__()
        if img_cross_attention_scale_learnable:
            raise NotImplementedError("img_cross_attention_scale_learnable (a learnable alpha on the image branch) is not used by the "
                                      "DynamiCrafter recipe (configs/002_dynamicrafter) and is not implemented")
        if fps_cond and fs_condition:
            raise ValueError("fps_cond (openaimodel3d.UNetModel) and fs_condition (openaimodel3d_dc.UNetModel) name the same fps_embedding")
        if not 0.0 <= dropout < 1.0:
            raise ValueError("dropout must be in [0, 1)")
        if in_channels > 8:
            raise NotImplementedError("the input convolution takes up to 8 channels (4 latent + 4 conditioning-frame channels)")
        unsupported = dict(use_scale_shift_norm=use_scale_shift_norm, resblock_updown=resblock_updown, tempspatial_aware=tempspatial_aware,
                           use_causal_attention=use_causal_attention, use_image_attention=use_image_attention,
                           not_use_linear=not use_linear, not_conv_resample=not conv_resample,
                           not_selfatt_only=not temporal_selfatt_only, depth=transformer_depth != 1 or temporal_transformer_depth != 1,
                           dims=dims != 2, num_heads=num_heads != -1)
        bad = [k for k, v in unsupported.items() if v]
        if bad:
            raise NotImplementedError(f"vt355 UNetModel implements the VideoCrafter1, VideoCrafter2 and DynamiCrafter recipes "
                                      f"(configs/000_videocrafter, configs/001_videocrafter2, configs/002_dynamicrafter); "
                                      f"unsupported options: {bad}")
        if num_head_channels != 64:
            raise NotImplementedError("the attention kernels are built for num_head_channels = 64")
        if model_channels % 64 or context_dim is None or context_dim % 64:
            raise ValueError("model_channels and context_dim must be multiples of 64 (one K-tile of the GEMM / convolution kernels)")
        if temporal_attention and (temporal_length is None or 32 % temporal_length):
            raise ValueError("temporal_length must divide 32 (packed temporal attention, csrc/attn_small.hip)")
        self.config = SimpleNamespace(in_channels=in_channels, model_channels=model_channels, out_channels=out_channels,
                                      num_res_blocks=num_res_blocks, attention_resolutions=tuple(attention_resolutions),
                                      channel_mult=tuple(channel_mult), context_dim=context_dim, num_head_channels=num_head_channels,
                                      temporal_conv=temporal_conv, temporal_attention=temporal_attention, temporal_length=temporal_length,
                                      addition_attention=addition_attention, fps_cond=fps_cond, use_checkpoint=use_checkpoint,
                                      text_context_len=text_context_len, img_cross_attention=bool(img_cross_attention),
                                      img_cross_attention_scale=1.0, img_context_len=16, default_fs=int(default_fs),
                                      fs_condition=bool(fs_condition), dropout=float(dropout),
                                      use_relative_position=bool(use_relative_position and temporal_attention))
        self.in_channels, self.model_channels, self.out_channels = in_channels, model_channels, out_channels
        self.tconv_dropout_p = 0.1          # TemporalConvBlock(dropout=0.1), hard-coded in ResBlock (openaimodel3d.py:205-210)
        self.dropout_seed: Optional[int] = None      # None: a fresh seed per training forward from torch's CPU generator
        self.last_emb = None                         # embedding sum [B, 4*model_channels] of the last forward (everything timesteps / fps / fs decide)
        self.last_dropout_sites: List = []           # (site name, counter offset, rows, channels) of the last training forward (tests)
        self.structure = build_structure(self.config)
        self._setup_flat(_param_shapes(self.config, self.structure))
        object.__setattr__(self, "lora", None)       # _UNetLora after add_lora(); a plain attribute: its parameters sit in THIS module's tree
        st_ = self.structure
        layers = [l for blk in st_.input + [st_.middle] + st_.output for l in blk] + ([st_.init_attn] if st_.init_attn is not None else [])
        self._temporal_owners = {l.pre for l in layers if l.kind == "tt"}

    # ---- LoRA (vc2_t2v_lora.yaml) ----
    def add_lora(self, r: int = 4, lora_alpha: float = 1.0, target_modules=LORA_TARGETS, seed: int = 0):
        """peft.get_peft_model's effect on this network: adapters on the target projections of every CrossAttention, every base weight frozen"""
        if self.config.img_cross_attention:
            raise NotImplementedError("LoRA on the image-conditioned UNet: the reference ships no such recipe")
        if self.train_state is not None:
            raise RuntimeError("add_lora() after enable_training(): the full fine-tune state already exists")
        if self.lora is not None:
            raise RuntimeError("adapters were already added")
        lora = _UNetLora(self, r, lora_alpha, target_modules)
        if self.flat_bf16.device != lora.flat_bf16.device or self.flat_bf16.dtype != lora.flat_bf16.dtype:
            for q in lora._plist.values():
                q.data = q.data.to(device=self.flat_bf16.device, dtype=self.flat_bf16.dtype)
            lora._reflat()
        object.__setattr__(self, "lora", lora)
        for q in self._plist.values():
            q.requires_grad_(False)
        lora.init_weights(seed)
        self._packed = None
        return self

    def enable_lora_training(self):
        """training state of the adapters only (hand it to FusedAdamW(ts.params, fullft_state=ts)); the base weights stay frozen"""
        if self.lora is None:
            raise RuntimeError("call add_lora(r, lora_alpha, target_modules) first")
        return self.lora.enable_training()

    def _apply(self, fn, *a, **k):
        if self.lora is not None and self.lora.train_state is not None:
            raise RuntimeError("move / convert the model BEFORE enable_lora_training()")
        out = super()._apply(fn, *a, **k)
        if self.lora is not None:
            self.lora._reflat()
        return out

    def load_state_dict(self, sd, strict: bool = True, **kw):
        out = super().load_state_dict(sd, strict=strict, **kw)
        if self.lora is not None:
            self.lora.weights_changed()
        return out

    def print_trainable_parameters(self):
        tr = sum(p.numel() for p in self.parameters() if p.requires_grad)
        al = sum(p.numel() for p in self.parameters())
        print(f"trainable params: {tr:,d} || all params: {al:,d} || trainable%: {100 * tr / max(al, 1):.4f}")

    def init_weights(self, seed: int = 0):
        """seeded random init for synthetic runs (no checkpoints offline); nothing is left at the reference's zero init"""
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for n, p in self._plist.items():
                shp = self.shapes[n]
                if len(shp) == 1:
                    w = torch.randn(shp, generator=g) * 0.1 + (1.0 if n.endswith("weight") else 0.0)
                elif n.endswith(".embeddings_table"):       # RelativePosition: xavier_uniform_ (attention.py:29), here its standard deviation
                    w = torch.randn(shp, generator=g) * math.sqrt(2.0 / (shp[0] + shp[1]))
                else:
                    w = torch.randn(shp, generator=g) * (0.7 / math.sqrt(math.prod(shp[1:])))
                p.copy_(w.to(p.device, BF16))
        self._packed = None
        return self

    # ---- forward ----
    def resolve_fs(self, fs, B: int, device):
        """the frame-stride / fps condition the network embeds: ``fs`` (int | int64 [B]), default_fs when None (openaimodel3d_dc.py:700-704)"""
        if fs is None:
            fs = self.config.default_fs
        if isinstance(fs, int):
            return torch.full((B,), fs, dtype=torch.int64, device=device)
        return fs.to(device=device, dtype=torch.int64)

    def forward(self, x, timesteps, context=None, features_adapter=None, fps=16, fs=None, **kwargs):
        """x [B, C, T, H, W] bf16, timesteps int64 [B], context [B, L, context_dim], fps int | int64 [B] -> [B, C_out, T, H, W]
        (openaimodel3d.py:650-694).  With fs_condition (openaimodel3d_dc.py:676-735) the frame-stride / fps condition is ``fs`` (int64 [B];
        None = default_fs) and ``fps`` is not read.  With img_cross_attention the context is [B, 77 + T*16, context_dim] (77 text tokens,
        then 16 image tokens per frame) or [B, 77 + n <= 32, context_dim] (one image set for all frames); when it requires grad, the
        gradient of its image rows comes back through autograd (the text rows get zeros: the text encoder is frozen)."""
        if features_adapter is not None:
            raise NotImplementedError("features_adapter is not part of the VideoCrafter2 training path")
        if not x.is_cuda:
            raise RuntimeError("vt355 UNetModel runs only on an MI355X device (no CPU fallback)")
        if x.dtype != BF16:
            raise TypeError(f"x must be bf16 (model dtype), got {x.dtype}")
        if context is None:
            raise ValueError("context (text embeddings [B, L, context_dim]) is required")
        B = x.shape[0]
        if self.config.fs_condition:
            fps = self.resolve_fs(fs, B, x.device)
        if isinstance(fps, int):
            fps = torch.full((B,), fps, dtype=torch.int64, device=x.device)
        need_grad = torch.is_grad_enabled() and (self.train_state is not None or (self.lora is not None and self.lora.train_state is not None))
        if need_grad:
            anchor = torch.zeros(1, device=x.device, requires_grad=True)
            return _UNetFn.apply(anchor, self, x, timesteps, context, fps)
        run = _Run(self, save=False)
        out, _ = run.forward(x, timesteps, context, fps)
        self.last_emb = run.emb
        return out


class _UNetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, model, x, t, context, fps):
        run = _Run(model, save=True)
        out, _ = run.forward(x, t, context, fps)
        model.last_dropout_sites = run.drop_sites
        model.last_emb = run.emb
        ctx.run = run
        return out

    @staticmethod
    def backward(ctx, dout):
        ctx.run.backward(dout)
        dctx = ctx.run.context_grad() if ctx.needs_input_grad[4] else None
        ctx.run = None
        return None, None, None, None, dctx, None


# ---------------------------------------------------------------------------------------------------------------------
# operand packing: what the kernels read besides the flat views (transposed / flipped copies for the input gradients)
# ---------------------------------------------------------------------------------------------------------------------
def _packed(model: UNetModel) -> SimpleNamespace:
    ver = -1 if model.train_state is None else model.train_state.version
    if model._packed is not None and model._packed_version == ver:
        return model._packed
    P = SimpleNamespace(wt={}, wdx={}, w={})
    fb = model.flat_bf16
    train = model.train_state is not None or (model.lora is not None and model.lora.train_state is not None)     # activation gradients flow either way
    # The transposed / flipped operand copies of ALL weights are refreshed by one launch (ops.TransposePlan): sources are views of the flat
    # parameter buffer, destinations are allocated once.  VT355_TRANSPOSE_PLAN=0: one launch per weight (A/B).
    tp = getattr(model, "_tplan", None)
    if tp is None or tp.key != (fb.data_ptr(), str(fb.device)):
        tp = model._tplan = SimpleNamespace(key=(fb.data_ptr(), str(fb.device)), plan=ops.TransposePlan(fb.device), wt={}, wdx={}, built=False)
    use_plan = fb.is_cuda and os.environ.get("VT355_TRANSPOSE_PLAN") != "0"
    with torch.no_grad():
        for n, shp in model.shapes.items():
            if not n.endswith("weight") or len(shp) == 1:
                continue
            if _is_conv(shp) and not (len(shp) == 4 and shp[2] == 1):            # 3x3 / (3,1,1) convolutions
                if train and n != "input_blocks.0.0.weight":
                    w = model._plist[n].detach()
                    if w.shape[0] % 64:         # out conv (4 output channels): its input-gradient conv reads dY padded to one K-tile
                        wp_ = torch.zeros((w.shape[0] + 63) // 64 * 64, *w.shape[1:], dtype=BF16, device=w.device)
                        wp_[:w.shape[0]] = w
                        P.wdx[n] = ops.pack_conv_weight_dx(wp_)
                    else:                       # one batched transpose of the tap-major storage [Cout, taps, Cin] (was flip + permute + contiguous)
                        o_ = model.offsets[n]
                        ws = fb[o_:o_ + math.prod(shp)].view(shp[0], math.prod(shp[2:]), shp[1])
                        if use_plan and n in tp.wdx:
                            P.wdx[n] = tp.wdx[n]
                        elif use_plan and not tp.built:
                            dst = torch.empty(shp[1], math.prod(shp[2:]) * shp[0], dtype=BF16, device=fb.device)
                            if tp.plan.add_conv_dx(ws, dst):
                                tp.wdx[n] = dst
                            else:
                                dst = ops.conv_weight_dx_from_storage(ws)
                            P.wdx[n] = dst
                        else:
                            P.wdx[n] = ops.conv_weight_dx_from_storage(ws)
            elif train:                                                          # Linear / 1x1 conv / Conv1d(k=1): [N, K]
                w2 = model.flat(fb, n)
                w2 = w2.reshape(w2.shape[0], -1)
                if use_plan and n in tp.wt:
                    P.wt[n] = tp.wt[n]
                elif use_plan and not tp.built:
                    dst = torch.empty(w2.shape[1], w2.shape[0], dtype=BF16, device=fb.device)
                    if tp.plan.add(w2, dst):
                        tp.wt[n] = dst
                    else:
                        dst = ops.transpose(w2)
                    P.wt[n] = dst
                else:
                    P.wt[n] = ops.transpose(w2)
        # conv_in: 4 input channels padded to one 64-channel K-tile
        w = model._plist["input_blocks.0.0.weight"].detach()                      # [mc, cin, 3, 3]
        wp = torch.zeros(w.shape[0], 3, 3, 64, dtype=BF16, device=w.device)
        wp[..., :w.shape[1]] = w.permute(0, 2, 3, 1)
        P.w["conv_in"] = wp.view(w.shape[0], -1)
        if use_plan and train:
            tp.built = True
            tp.plan.run()
    model._packed, model._packed_version = P, ver
    return P


def _lora_packed(model: UNetModel) -> SimpleNamespace:
    """Per adapted Linear call of the engine (key = its first weight name): the K-extension of DESIGN 3 "LoRA as a K-extension" --
    W_ext [N, K + EXT] = [W | scaling B (adapter j in columns j r .. of its row block) | 0] and its transpose, A3 [EXT, K] (rows j r ..: A_j)
    and its transpose, so that y = [x | x A3^T] W_ext^T is ONE GEMM.  A call is one projection (to_q of a text cross-attention) or several
    adjacent ones sharing their input (to_q | to_k | to_v of a self-attention, to_k | to_v on the context).  Rebuilt when the adapters change."""
    L = model.lora
    ver = -1 if L.train_state is None else L.train_state.version
    if L._packed is not None and L._packed_version == ver:
        return L._packed
    # the frozen base weight fills all but 64 columns of W_ext: while only the ADAPTERS change (the base pack `_packed(model)` is the same object)
    # the previous W_ext / W_ext^T are kept and only their extension columns / rows and A3 are rewritten
    base_key = id(_packed(model))
    prev = L._packed if (L._packed is not None and getattr(L, "_packed_base", None) == base_key) else None
    P = prev if prev is not None else SimpleNamespace(wext={}, wtext={}, a3={}, a3t={}, mods={})
    r = L.r
    sites = set(L.sites)
    names = list(model.shapes)
    with torch.no_grad():
        for att in sorted({m.rsplit(".", 1)[0] for m in L.sites} | {n[:-len(".to_q.weight")] for n in names if n.endswith(".to_q.weight")}):
            calls = [[att + ".to_q", att + ".to_k", att + ".to_v"]] if _is_self(model, att) else [[att + ".to_q"], [att + ".to_k", att + ".to_v"]]
            for mods in calls:
                if not any(m in sites for m in mods):
                    continue
                K = model.shapes[mods[0] + ".weight"][1]
                key = mods[0] + ".weight"
                if prev is None:
                    w = model.span(model.flat_bf16, mods[0] + ".weight", mods[-1] + ".weight")
                    wext = torch.zeros(w.shape[0], K + EXT, dtype=BF16, device=w.device)
                    wext[:, :K] = w
                    wtext = torch.zeros(K + EXT, w.shape[0], dtype=BF16, device=w.device)
                    wtext[:K] = ops.transpose(w)
                    P.wext[key], P.wtext[key] = wext, wtext
                    P.a3[key] = torch.zeros(EXT, K, dtype=BF16, device=w.device)
                    P.a3t[key] = torch.zeros(K, EXT, dtype=BF16, device=w.device)
                    P.mods[key] = mods
                wext, wtext, a3, a3t = P.wext[key], P.wtext[key], P.a3[key], P.a3t[key]
                row = 0
                for j, m in enumerate(mods):
                    n_out = model.shapes[m + ".weight"][0]
                    if m in sites:
                        sb = (L._plist[m + ".lora_B.default.weight"].float() * L.scaling).to(BF16)          # [n_out, r]
                        wext[row:row + n_out, K + j * r:K + (j + 1) * r] = sb
                        wtext[K + j * r:K + (j + 1) * r, row:row + n_out] = sb.t()
                        a = L._plist[m + ".lora_A.default.weight"]                                         # [r, K]
                        a3[j * r:(j + 1) * r] = a
                        a3t[:, j * r:(j + 1) * r] = a.t()
                    row += n_out
    L._packed_base = base_key
    L._packed, L._packed_version = P, ver
    return P


def _is_self(model: UNetModel, att: str) -> bool:
    """does the engine run this CrossAttention as a self-attention (one fused q | k | v projection of its input)?  Everything except the
    text cross-attention attn2 of a SPATIAL transformer block (the temporal blocks are self-attention only: temporal_selfatt_only)"""
    if not att.endswith(".attn2"):
        return True
    owner = att.split(".transformer_blocks.")[0]
    return owner in model._temporal_owners


_TRACE = {"f": None}


def _trace_file():
    import os
    path = os.environ.get("VT_UNET_TRACE")
    if not path:
        return None
    if _TRACE["f"] is None:
        _TRACE["f"] = open(path, "a")
    return _TRACE["f"]


class _Var:
    """an activation [rows, C] (bf16, row stride may exceed C) and, during the backward pass, its gradient"""
    __slots__ = ("d", "g", "ext", "shared", "g32", "gq")

    def __init__(self, d, ext=None, shared=False):
        self.d, self.g, self.ext = d, None, ext          # ext: the [rows, C + EXT] buffer d is the first C columns of (input of a LoRA'd Linear)
        self.g32 = None                                  # fp32 accumulator for a gradient summed over many layers (the image context)
        self.gq = None                                   # fp8 copy of g left by its producer for an fp8 dX product (HunyuanVideo fp8_dgrad)
        self.shared = shared                             # several adapted Linears read this buffer (the text context): each keeps its own x A^T


class _Run:
    # defaults for the engines that subclass this tape (vt355.stdit, vt355.hunyuan) and set up their own state
    frozen = False
    lora = LP = lts = drop = None
    _img_ctx = None
    _dual_ws = None

    def __init__(self, model: UNetModel, save: bool):
        self.m, self.save = model, save
        self.c = model.config
        self.P = _packed(model)
        self.fb = model.flat_bf16
        self.ts = model.train_state
        self.tape: List = []
        self.dev = model.device
        # LoRA mode: the base weights are frozen (self.ts is None: no gradient buffers, no dW work); the adapters' state is self.lts
        self.lora = model.lora
        self.LP = _lora_packed(model) if model.lora is not None else None
        self.lts = None if model.lora is None else model.lora.train_state
        self.frozen = self.ts is None
        # train-mode dropout (module docstring): (p, seed) or None; site k of this forward uses the counter range starting at k << 36
        self.drop = None
        if save and model.training and model.tconv_dropout_p > 0.0:
            seed = model.dropout_seed if model.dropout_seed is not None else int(torch.randint(0, 2 ** 62, (1,)).item())
            self.drop = (float(model.tconv_dropout_p), int(seed))
        self.drop_sites: List = []

    # ---- small helpers ----
    def E(self, *s, dt=BF16):
        return torch.empty(*s, dtype=dt, device=self.dev)

    def W(self, name):
        return self.m.flat(self.fb, name)

    def G(self, name):
        return None if self.frozen else self.m.flat(self.ts.grad, name)

    def act(self, M, C, ext: bool):
        """activation buffer [M, C]; ext (input of an adapted Linear in LoRA mode): the first C columns of a [M, C + EXT] buffer"""
        if ext and self.lora is not None:
            full = self.E(M, C + EXT)
            return full[:, :C], full
        return self.E(M, C), None

    def acc(self, v: _Var, g):
        if v.g32 is not None:
            v.g32.add_(g)
        elif v.g is None:
            v.g = g
        else:
            ops.add_rows(v.g, g, v.g)

    def dW(self, dy, x, name_or_tensor, dbias=None):
        """weight gradient of a Linear (+ its bias gradient dbias += column sums of dy: folded into the 320-row kernel's pass over dy where that runs)"""
        if self.frozen:
            return
        dw = self.G(name_or_tensor) if isinstance(name_or_tensor, str) else name_or_tensor
        P_, Q_ = dw.shape
        # outputs in multiples of 320 (every VC2 width): the one-tap weight-gradient convolution's 320-row kernel beats the 128-tile GEMM
        # at 8 of the 10 UNet shapes (profiles/r03_dw_kbench.txt: 640 x 640 over 40 960 rows 69 vs 98 us)
        if P_ % 128 == 0 and Q_ % 128 == 0 and dy.shape[0] >= 256 and not (P_ % 320 == 0 and dy.shape[0] >= 2048):
            ops.gemm_nt(dy, x, dw, P=P_, Q=Q_)
            if dbias is not None:
                ops.group_colsum(dy, dbias, D=P_)
        else:
            ops.linear_dw(dy, x, dw, accumulate=True, dbias=dbias)

    # ---- layers: each returns the output _Var and (when saving) pushes its backward onto the tape ----
    def linear(self, x: _Var, wname: str, bname: Optional[str], residual: Optional[_Var] = None, wspan=None, out=None) -> _Var:
        """y = x W^T + b (+ residual).  wspan = (first, last): several adjacent matrices as one (fused q|k|v)"""
        key = wspan[0] if wspan else wname
        if self.lora is not None and key in self.LP.wext:
            assert bname is None and residual is None and out is None
            return self.lora_linear(x, key)
        w = self.m.span(self.fb, *wspan) if wspan else self.W(wname)
        if w.dim() == 3:
            w = w.view(w.shape[0], -1)
        M = x.d.shape[0]
        y = out if out is not None else self.E(M, w.shape[0])
        b = None if bname is None else self.W(bname)
        if ops.rows320(w.shape[0], M, w.shape[1]) and w.is_contiguous():
            ops.linear_rows(x.d, w, y, b, None if residual is None else residual.d)
        elif residual is not None:
            ops.gemm(x.d, w, y, b, epilogue=EPI_GATED_RES, residual=residual.d)
        else:
            ops.gemm(x.d, w, y, b)
        yv = _Var(y)
        if self.save:
            def bwd():
                g = yv.g
                if residual is not None:
                    self.acc(residual, g)
                db = self.G(bname) if (bname is not None and not self.frozen) else None
                if wspan:
                    wt = self._wt_span(wspan)
                    if not self.frozen:
                        o0 = self.m.offsets[wspan[0]]
                        self.dW(g, x.d, self.ts.grad[o0:o0 + w.numel()].view(w.shape), dbias=db)
                else:
                    wt = self.P.wt[wname]
                    if not self.frozen:
                        dw = self.G(wname)
                        if dw.dim() == 3:
                            dw = dw.view(dw.shape[0], -1)
                        self.dW(g, x.d, dw, dbias=db)
                if x is not None and x.g is not False:
                    dx = self.E(M, w.shape[1])
                    if ops.rows320(w.shape[1], M, w.shape[0]):
                        ops.linear_rows(g, wt, dx)
                    else:
                        ops.gemm(g, wt, dx, None)
                    self.acc(x, dx)
            self.tape.append(bwd)
        return yv

    def lora_linear(self, x: _Var, key: str) -> _Var:
        """y = [x | x A3^T] W_ext^T for the adapted projection(s) `key` (no bias: to_q / to_k / to_v have none); x.ext holds x in its first
        K columns.  Backward: [dx | dt] = g W_ext; d(scaling B_j) = g_j^T t_j; dA_j = dt_j^T x; dx += dt A3 -- all through the stock GEMMs."""
        if x.ext is None:
            raise RuntimeError(f"{key}: the input of an adapted Linear must live in an extended buffer (engine bug)")
        LP, L = self.LP, self.lora
        wext, a3 = LP.wext[key], LP.a3[key]
        K = wext.shape[1] - EXT
        xe = x.ext
        M = xe.shape[0]
        ops.gemm(xe[:, :K], a3, xe[:, K:], None, K=K)                  # t = x A3^T into the extension columns
        y = self.E(M, wext.shape[0])
        ops.gemm(xe, wext, y, None)
        # the context buffer serves every text cross-attention: the next one overwrites the extension columns, so this call keeps its t
        t_ext = xe[:, K:].clone() if (x.shared and self.save) else xe[:, K:]
        yv = _Var(y)
        if self.save:
            def bwd_lora():
                g = yv.g
                r = L.r
                dxe = self.E(M, K + EXT)
                ops.gemm(g, LP.wtext[key], dxe, None)                   # [dx | dt] = g W_ext
                if self.lts is not None:
                    db = torch.zeros(wext.shape[0], EXT, dtype=F32, device=self.dev)
                    ops.linear_dw(g, t_ext, db, accumulate=False)           # d(scaling B) blocks = g^T t
                    da = torch.zeros(EXT, K, dtype=F32, device=self.dev)
                    ops.linear_dw(dxe[:, K:], xe[:, :K], da, accumulate=False)   # dA3 = dt^T x
                    row = 0
                    for j, mod in enumerate(LP.mods[key]):
                        n_out = self.m.shapes[mod + ".weight"][0]
                        if mod in L.shapes_sites:
                            L.flat(self.lts.grad, mod + ".lora_B.default.weight").add_(db[row:row + n_out, j * r:(j + 1) * r], alpha=L.scaling)
                            L.flat(self.lts.grad, mod + ".lora_A.default.weight").add_(da[j * r:(j + 1) * r])
                        row += n_out
                if x.g is not False:
                    dx = self.E(M, K)
                    ops.gemm(dxe[:, K:], LP.a3t[key], dx, None, epilogue=EPI_GATED_RES, residual=dxe[:, :K])     # dx + dt A3
                    self.acc(x, dx)
            self.tape.append(bwd_lora)
        return yv

    def _wt_span(self, wspan):
        key = "span:" + wspan[0]
        if key not in self.P.wt:
            self.P.wt[key] = ops.transpose(self.m.span(self.fb, *wspan))
        return self.P.wt[key]

    def groupnorm(self, x: _Var, pre: str, N: int, eps: float, silu: bool) -> _Var:
        """x [N*P, C] as N samples of P positions"""
        M, C = x.d.shape
        P_ = M // N
        y = self.E(M, C)
        x3 = x.d.view(N, P_, C) if x.d.is_contiguous() else x.d.as_strided((N, P_, C), (P_ * x.d.stride(0), x.d.stride(0), 1))
        ws = ops.groupnorm_fwd(x3, self.W(pre + ".weight"), self.W(pre + ".bias"), y.view(N, P_, C), 32, eps, silu)
        yv = _Var(y)
        if self.save:
            def bwd():
                g = yv.g
                g3 = g.view(N, P_, C) if g.is_contiguous() else g.as_strided((N, P_, C), (P_ * g.stride(0), g.stride(0), 1))
                if x.g is None:
                    dx = self.E(M, C)
                    ops.groupnorm_bwd(g3, x3, self.W(pre + ".weight"), ws, dx.view(N, P_, C), self.G(pre + ".weight"), self.G(pre + ".bias"), 32, silu)
                    x.g = dx
                else:
                    xg = x.g
                    xg3 = xg.view(N, P_, C) if xg.is_contiguous() else xg.as_strided((N, P_, C), (P_ * xg.stride(0), xg.stride(0), 1))
                    ops.groupnorm_bwd(g3, x3, self.W(pre + ".weight"), ws, xg3, self.G(pre + ".weight"), self.G(pre + ".bias"), 32, silu,
                                      accumulate=True)
            self.tape.append(bwd)
        return yv

    def dropout(self, x: _Var, site: str, p: Optional[float] = None) -> _Var:
        """nn.Dropout(p) in training mode; the backward pass re-derives the mask from (seed, offset)"""
        if self.drop is None:
            return x
        p_, seed = self.drop
        if p is not None:
            p_ = float(p)
        off = len(self.drop_sites) << 36
        M, C = x.d.shape
        self.drop_sites.append((site, off, M, C))
        y = self.E(M, C)
        ops.dropout(x.d, y, p_, seed, off)
        yv = _Var(y)

        def bwd():
            g = self.E(M, C)
            ops.dropout(yv.g, g, p_, seed, off)
            self.acc(x, g)
        self.tape.append(bwd)
        return yv

    def layernorm(self, x: _Var, pre: str, ext: bool = False) -> _Var:
        """ext: the output feeds adapted projections (LoRA mode): it is written into the first D columns of an extended buffer"""
        M, D = x.d.shape
        y, yext = self.act(M, D, ext)
        mean, rstd = self.E(M, dt=F32), self.E(M, dt=F32)
        ga, be = self.W(pre + ".weight"), self.W(pre + ".bias")
        ops.ln_modulate_fwd(x.d, y, ga, be, None, mean, rstd, D, 1, 0, 1e-5)
        yv = _Var(y, yext)
        if self.save:
            def bwd():
                g = yv.g
                if not self.frozen:
                    G12 = torch.zeros(2, 1, D, dtype=F32, device=self.dev)        # one fill for both sums
                    G1, G2 = G12[0], G12[1]
                    ops.group_colsum(g, G1, y=x.d, out2=G2, mean=mean, rstd=rstd, D=D)
                    ops.ln_param_combine(G1, G2, D, ga, be, None, self.G(pre + ".weight"), self.G(pre + ".bias"), None, False)
                dx = self.E(M, D)
                ops.ln_modulate_bwd(g, x.d, mean, rstd, ga, None, x.g, dx, D, 1, 0)     # dx = (earlier gradient of x) + LN'(g)
                x.g = dx
            self.tape.append(bwd)
        return yv

    def self_attention_spatial(self, x: _Var, pre: str, heads: int, nseq: int, residual: _Var) -> _Var:
        """CrossAttention with context None over nseq sequences of M/nseq rows (attention.py:101-181) + residual"""
        M, C = x.d.shape
        S = M // nseq
        qkv = self.linear(x, None, None, wspan=(pre + ".to_q.weight", pre + ".to_v.weight"))
        o = self.E(M, C)
        lse = self.E(nseq, heads, S, dt=F32)
        q3 = qkv.d.view(nseq, S, 3 * C)
        ops.attn_fwd(q3[:, :, :C], q3[:, :, C:2 * C], q3[:, :, 2 * C:], o.view(nseq, S, C), lse, nseq, heads, S, scale=0.125)
        ov = _Var(o)
        if self.save:
            def bwd():
                g = ov.g
                dqkv = self.E(M, 3 * C)
                dq = torch.zeros(nseq, S, C, dtype=F32, device=self.dev)
                delta = self.E(nseq * heads * S, dt=F32)
                d3 = dqkv.view(nseq, S, 3 * C)
                ops.attn_bwd(q3[:, :, :C], q3[:, :, C:2 * C], q3[:, :, 2 * C:], o.view(nseq, S, C), g.view(nseq, S, C), lse, delta, dq,
                             d3[:, :, C:2 * C], d3[:, :, 2 * C:], nseq, heads, S, scale=0.125,
                             chain_ws=ops.attn_bwd_chain_workspace(nseq, heads, S, self.dev))
                ops.residual_cast(dq.view(M, C), None, dqkv[:, :C])
                qkv.g = dqkv
            self.tape.append(bwd)
        return self.linear(ov, pre + ".to_out.0.weight", pre + ".to_out.0.bias", residual=residual)

    def attention_packed(self, x: _Var, pre: str, heads: int, T: int, residual: _Var) -> _Var:
        """temporal self-attention: rows are consecutive sequences of T (attention.py:395-519; both attn1 and attn2)"""
        M, C = x.d.shape
        qkv = self.linear(x, None, None, wspan=(pre + ".to_q.weight", pre + ".to_v.weight"))
        o = self.E(M, C)
        lse = self.E(1, heads, M, dt=F32)
        q3 = qkv.d.view(1, M, 3 * C)
        if self.c.use_relative_position:
            return self._attention_relpos(qkv, o, lse, pre, heads, T, residual)
        ops.attn_small_fwd(q3[:, :, :C], q3[:, :, C:2 * C], q3[:, :, 2 * C:], o.view(1, M, C), lse, heads, 0.125, mask_block=T)
        ov = _Var(o)
        if self.save:
            def bwd():
                dqkv = self.E(M, 3 * C)
                d3 = dqkv.view(1, M, 3 * C)
                ops.attn_small_bwd(q3[:, :, :C], q3[:, :, C:2 * C], q3[:, :, 2 * C:], o.view(1, M, C), ov.g.view(1, M, C), lse,
                                   d3[:, :, :C], d3[:, :, C:2 * C], d3[:, :, 2 * C:], heads, 0.125, mask_block=T)
                qkv.g = dqkv
            self.tape.append(bwd)
        return self.linear(ov, pre + ".to_out.0.weight", pre + ".to_out.0.bias", residual=residual)

    def _attention_relpos(self, qkv: _Var, o, lse, pre: str, heads: int, T: int, residual: _Var) -> _Var:
        """attention_packed with CrossAttention(relative_position=True)'s two tables (attention.py:126-149; csrc/attn_relpos.hip).  The
        tables are parameters: their gradients are added into the flat gradient buffer (full fine-tune) or skipped (frozen base, LoRA)"""
        M, C = o.shape
        tk, tv = pre + ".relative_position_k.embeddings_table", pre + ".relative_position_v.embeddings_table"
        q, k, v = qkv.d[:, :C], qkv.d[:, C:2 * C], qkv.d[:, 2 * C:]
        ops.attn_relpos_fwd(q, k, v, self.W(tk), self.W(tv), o, lse.view(heads, M), heads, T, 0.125)
        ov = _Var(o)
        if self.save:
            def bwd():
                dqkv = self.E(M, 3 * C)
                ops.attn_relpos_bwd(q, k, v, self.W(tk), self.W(tv), o, ov.g, lse.view(heads, M), dqkv[:, :C], dqkv[:, C:2 * C],
                                    dqkv[:, 2 * C:], self.G(tk), self.G(tv), heads, T, 0.125)
                qkv.g = dqkv
            self.tape.append(bwd)
        return self.linear(ov, pre + ".to_out.0.weight", pre + ".to_out.0.bias", residual=residual)

    def cross_attention(self, x: _Var, pre: str, heads: int, B: int, ctx: _Var, L: int, residual: _Var, img=None) -> _Var:
        """text cross-attention: the M/B rows of a sample against its L context rows (attention.py:101-181, context[:, :77]).
        img = (image context _Var [NI*Sb, ctx], NI, Sb): the image branch of CrossAttention(img_cross_attention=True) -- a second softmax
        over the Sb image keys of the query's frame (NI = B*T items) or of its sample (NI = B), added to the text result"""
        M, C = x.d.shape
        q = self.linear(x, pre + ".to_q.weight", None)
        kv = self.linear(ctx, None, None, wspan=(pre + ".to_k.weight", pre + ".to_v.weight"))        # [B*L, 2C]
        if img is not None:
            return self._dual_attention(x, pre, heads, B, q, kv, L, residual, *img)
        o = self.E(M, C)
        lse = self.E(B, heads, M // B, dt=F32)
        kv3 = kv.d.view(B, L, 2 * C)
        ops.attn_small_fwd(q.d.view(B, M // B, C), kv3[:, :, :C], kv3[:, :, C:], o.view(B, M // B, C), lse, heads, 0.125)
        ov = _Var(o)
        if self.save:
            def bwd():
                dq = self.E(M, C)
                dk = self.E(B, L, C, dt=F32); dv = self.E(B, L, C, dt=F32)
                ops.attn_small_bwd(q.d.view(B, M // B, C), kv3[:, :, :C], kv3[:, :, C:], o.view(B, M // B, C), ov.g.view(B, M // B, C), lse,
                                   dq.view(B, M // B, C), dk, dv, heads, 0.125)
                q.g = dq
                dkv = self.E(B * L, 2 * C)
                ops.residual_cast(dk.view(B * L, C), None, dkv[:, :C])
                ops.residual_cast(dv.view(B * L, C), None, dkv[:, C:])
                kv.g = dkv
            self.tape.append(bwd)
        return self.linear(ov, pre + ".to_out.0.weight", pre + ".to_out.0.bias", residual=residual)

    def _dual_attention(self, x, pre, heads, B, q, kv, L, residual, imgv, NI, Sb) -> _Var:
        M, C = x.d.shape
        Sq = M // B
        rpf = Sq // (NI // B)                       # rows of one frame at this level (NI == B: one image set per sample)
        kvi = self.linear(imgv, None, None, wspan=(pre + ".to_k_ip.weight", pre + ".to_v_ip.weight"))          # [NI*Sb, 2C]
        o = self.E(M, C)
        lse = self.E(2, B, heads, Sq, dt=F32)
        q3, o3 = q.d.view(B, Sq, C), o.view(B, Sq, C)
        kv3, kvi3 = kv.d.view(B, L, 2 * C), kvi.d.view(NI, Sb, 2 * C)
        c_img = float(self.c.img_cross_attention_scale)
        ops.attn_dual_fwd(q3, kv3[:, :, :C], kv3[:, :, C:], kvi3[:, :, :C], kvi3[:, :, C:], o3, lse, heads, 0.125, rpf, c_img)
        ov = _Var(o)
        if self.save:
            def bwd():
                dq = self.E(M, C)
                dk = self.E(B, L, C, dt=F32); dv = self.E(B, L, C, dt=F32)
                dki = self.E(NI, Sb, C, dt=F32); dvi = self.E(NI, Sb, C, dt=F32)
                need = ops.attn_dual_ws_floats(B, heads, Sq, rpf, L, Sb)
                if self._dual_ws is None or self._dual_ws.numel() < need:          # one scratch buffer for all blocks of the run (grows to the largest level)
                    self._dual_ws = self.E(max(need, 1), dt=F32)
                ops.attn_dual_bwd(q3, kv3[:, :, :C], kv3[:, :, C:], kvi3[:, :, :C], kvi3[:, :, C:], ov.g.view(B, Sq, C), lse,
                                  dq.view(B, Sq, C), dk, dv, dki, dvi, heads, 0.125, rpf, c_img, ws=self._dual_ws)
                q.g = dq
                dkv = self.E(B * L, 2 * C)
                ops.residual_cast(dk.view(B * L, C), None, dkv[:, :C])
                ops.residual_cast(dv.view(B * L, C), None, dkv[:, C:])
                kv.g = dkv
                dkvi = self.E(NI * Sb, 2 * C)
                ops.residual_cast(dki.view(NI * Sb, C), None, dkvi[:, :C])
                ops.residual_cast(dvi.view(NI * Sb, C), None, dkvi[:, C:])
                kvi.g = dkvi
            self.tape.append(bwd)
        return self.linear(ov, pre + ".to_out.0.weight", pre + ".to_out.0.bias", residual=residual)

    def feed_forward(self, x: _Var, pre: str, residual: _Var) -> _Var:
        h = self.linear(x, pre + ".net.0.proj.weight", pre + ".net.0.proj.bias")
        M, F2 = h.d.shape
        y = self.E(M, F2 // 2)
        ops.geglu_fwd(h.d, y)
        yv = _Var(y)
        if self.save:
            def bwd():
                dh = self.E(M, F2)
                ops.geglu_bwd(yv.g, h.d, dh)
                h.g = dh
            self.tape.append(bwd)
        return self.linear(yv, pre + ".net.2.weight", pre + ".net.2.bias", residual=residual)

    def conv(self, x5, wname: str, bname: str, kernel, padding, stride=1, sbias=None, residual5=None, wk=None, cin=None):
        """x5: bf16 [B,T,H,W,Cin] view; returns (y5, backward closure factory) -- the caller wraps the Vars"""
        wk_ = wk if wk is not None else self.W(wname)
        B, T, H, W_, _ = x5.shape
        Ho, Wo = (H + 2 * padding[1] - kernel[1]) // stride + 1, (W_ + 2 * padding[2] - kernel[2]) // stride + 1
        Cout = wk_.shape[0]
        ld = Cout if Cout % 8 == 0 else (Cout + 7) // 8 * 8
        y5 = self.E(B, T, Ho, Wo, ld)[..., :Cout]
        ops.conv_cl(x5, wk_, y5, kernel, padding, stride, bias=self.W(bname), sbias=sbias, residual=residual5)
        return y5

    def conv_bwd(self, g5, x5, wname, bname, kernel, padding, stride, need_dx=True, cin_true=None):
        """parameter gradients of a convolution and (returned) the gradient of its input"""
        Cout = g5.shape[4]
        g2 = g5.as_strided((g5.shape[0] * g5.shape[1] * g5.shape[2] * g5.shape[3], Cout), (g5.stride(3), 1))      # rows x channels view (row stride may exceed Cout)
        if self.frozen:
            pass                                # LoRA mode: the convolution weights do not train
        elif cin_true is None:
            ops.conv_dw_cl(g5, x5, self.G(wname), kernel, padding, stride, accumulate=True, dbias=self.G(bname))
        else:      # conv_in: 4 real input channels; the kernel wants whole 16-byte chunks per tap -> gradient against 8 channels, 4 kept
            ops.group_colsum(g2, self.G(bname), D=Cout)
            dw = self.G(wname)
            taps = kernel[0] * kernel[1] * kernel[2]
            tmp = torch.empty(Cout, taps * 8, dtype=F32, device=self.dev)
            ops.conv_dw_cl(g5, x5[..., :8], tmp, kernel, padding, stride, accumulate=False)
            dw.view(Cout, taps, cin_true).add_(tmp.view(Cout, taps, 8)[..., :cin_true])
        if not need_dx:
            return None
        B, T, H, W_, Cin = x5.shape
        dx5 = self.E(B, T, H, W_, Cin)
        if Cout % 64:                     # pad dY's channels to a whole K-tile (weights were padded alike in _packed)
            gp = torch.zeros(*g5.shape[:4], (Cout + 63) // 64 * 64, dtype=BF16, device=self.dev)
            gp[..., :Cout] = g5
            g5, Cout = gp, gp.shape[4]
            g2 = g5.view(-1, Cout)
        if stride == 1:
            ops.conv_cl(g5, self.P.wdx[wname], dx5, kernel, padding, 1)
        else:
            z = self.E(B, T, H, W_, Cout)
            ops.row_map(g2, z.view(-1, Cout), 2, B * T, g5.shape[2], g5.shape[3])
            ops.conv_cl(z, self.P.wdx[wname], dx5, kernel, padding, 1)
        return dx5

    # ---- blocks ----
    def res_block(self, l, x: _Var, shape, se: _Var, demb) -> _Var:
        """ResBlock._forward + TemporalConvBlock (openaimodel3d.py:229-310).  x rows = [B,T,H,W]; se = SiLU(emb) [B, te]"""
        B, T, H, W_ = shape
        pre, ci, co = l.pre, l.cin, l.cout
        M = B * T * H * W_
        k2, p2, kt, pt = (1, 3, 3), (0, 1, 1), (3, 1, 1), (1, 0, 0)
        x5 = x.d.view(B, T, H, W_, ci)
        h0 = self.groupnorm(x, pre + ".in_layers.0", B * T, 1e-5, True)
        eo = self.E(B, co, dt=F32)
        ops.gemm(se.d, self.W(pre + ".emb_layers.1.weight"), eo, self.W(pre + ".emb_layers.1.bias"))       # emb_out, fp32 [B, co]
        h1d = self.conv(h0.d.view(B, T, H, W_, ci), pre + ".in_layers.2.weight", pre + ".in_layers.2.bias", k2, p2, sbias=eo)
        h1 = _Var(h1d.view(M, co))
        if self.save:
            def bwd1():
                g5 = h1.g.view(B, T, H, W_, co)
                # emb_out gradient: per-sample column sums of dh -> Linear(SiLU(emb)) backward (few rows: vt_small_linear_bwd)
                if not self.frozen:          # (LoRA mode: nothing on the embedding path trains)
                    deo = torch.zeros(B, co, dtype=F32, device=self.dev)
                    ops.group_colsum(h1.g, deo, D=co, S=T * H * W_, St=0, grouped=True, o_bstride=co, o_segstride=0)
                    ops.small_linear_bwd(deo, se.d, self.W(pre + ".emb_layers.1.weight"), self.G(pre + ".emb_layers.1.weight"),
                                         self.G(pre + ".emb_layers.1.bias"), demb)
                h0.g = self.conv_bwd(g5, h0.d.view(B, T, H, W_, ci), pre + ".in_layers.2.weight", pre + ".in_layers.2.bias", k2, p2, 1).view(M, ci)
            self.tape.append(bwd1)
        h2 = self.groupnorm(h1, pre + ".out_layers.0", B * T, 1e-5, True)
        if self.c.dropout > 0.0:
            h2 = self.dropout(h2, pre + ".out_layers.2", p=self.c.dropout)      # ResBlock's nn.Dropout(p=dropout) (openaimodel3d.py:186-192)
        if ci != co:
            skip = self.linear(x, pre + ".skip_connection.weight", pre + ".skip_connection.bias")
        else:
            skip = x
        h3d = self.conv(h2.d.view(B, T, H, W_, co), pre + ".out_layers.3.weight", pre + ".out_layers.3.bias", k2, p2,
                        residual5=skip.d.view(B, T, H, W_, co))
        h3 = _Var(h3d.view(M, co))
        if self.save:
            def bwd2():
                g5 = h3.g.view(B, T, H, W_, co)
                self.acc(skip, h3.g)
                h2.g = self.conv_bwd(g5, h2.d.view(B, T, H, W_, co), pre + ".out_layers.3.weight", pre + ".out_layers.3.bias", k2, p2, 1).view(M, co)
            self.tape.append(bwd2)
        if not l.tconv:
            return h3
        cur = h3
        for j in (1, 2, 3, 4):
            last = 2 if j == 1 else 3
            pj = pre + f".temopral_conv.conv{j}"
            gn = self.groupnorm(cur, pj + ".0", B, 1e-5, True)
            if j > 1:
                gn = self.dropout(gn, pj)          # conv2..conv4: GroupNorm -> SiLU -> Dropout(0.1) -> Conv3d (openaimodel3d.py:283-300)
            yd = self.conv(gn.d.view(B, T, H, W_, co), pj + f".{last}.weight", pj + f".{last}.bias", kt, pt,
                           residual5=h3.d.view(B, T, H, W_, co) if j == 4 else None)
            nxt = _Var(yd.view(M, co))
            if self.save:
                def bwdt(nxt=nxt, gn=gn, pj=pj, last=last, j=j):
                    g5 = nxt.g.view(B, T, H, W_, co)
                    if j == 4:
                        self.acc(h3, nxt.g)
                    gn.g = self.conv_bwd(g5, gn.d.view(B, T, H, W_, co), pj + f".{last}.weight", pj + f".{last}.bias", kt, pt, 1).view(M, co)
                self.tape.append(bwdt)
            cur = nxt
        return cur

    def basic_block(self, x: _Var, pre: str, heads: int, mode: str, **kw) -> _Var:
        """BasicTransformerBlock._forward (attention.py:299-310)"""
        b = pre + ".transformer_blocks.0."
        if mode == "spatial":
            x = self.self_attention_spatial(self.layernorm(x, b + "norm1", ext=True), b + "attn1", heads, kw["nseq"], x)
            x = self.cross_attention(self.layernorm(x, b + "norm2", ext=True), b + "attn2", heads, kw["B"], kw["ctx"], kw["L"], x, img=kw.get("img"))
        else:
            x = self.attention_packed(self.layernorm(x, b + "norm1", ext=True), b + "attn1", heads, kw["T"], x)
            x = self.attention_packed(self.layernorm(x, b + "norm2", ext=True), b + "attn2", heads, kw["T"], x)
        return self.feed_forward(self.layernorm(x, b + "norm3"), b + "ff", x)

    def spatial_transformer(self, l, x: _Var, shape, ctx: _Var, L: int, img=None) -> _Var:
        B, T, H, W_ = shape
        n = self.groupnorm(x, l.pre + ".norm", B * T, 1e-6, False)
        h = self.linear(n, l.pre + ".proj_in.weight", l.pre + ".proj_in.bias")
        h = self.basic_block(h, l.pre, l.heads, "spatial", nseq=B * T, B=B, ctx=ctx, L=L, img=img)
        return self.linear(h, l.pre + ".proj_out.weight", l.pre + ".proj_out.bias", residual=x)

    def temporal_transformer(self, l, x: _Var, shape) -> _Var:
        B, T, H, W_ = shape
        M, C = x.d.shape
        n = self.groupnorm(x, l.pre + ".norm", B, 1e-6, False)
        nt = self.E(M, C)
        ops.row_map(n.d, nt, 0, B, T, H * W_)                      # [B, T, HW] -> [B, HW, T] rows
        ntv = _Var(nt)
        if self.save:
            def bwd_in():
                g = self.E(M, C)
                ops.row_map(ntv.g, g, 0, B, H * W_, T)
                n.g = g
            self.tape.append(bwd_in)
        h = self.linear(ntv, l.pre + ".proj_in.weight", l.pre + ".proj_in.bias")
        h = self.basic_block(h, l.pre, l.heads, "temporal", T=T)
        o = self.linear(h, l.pre + ".proj_out.weight", l.pre + ".proj_out.bias")
        y = self.E(M, C)
        ops.row_map(o.d, y, 0, B, H * W_, T)                       # back to [B, T, HW] rows ...
        ops.add_rows(y, x.d, y)                                    # ... + x_in
        yv = _Var(y)
        if self.save:
            def bwd_out():
                g = self.E(M, C)
                ops.row_map(yv.g, g, 0, B, T, H * W_)
                o.g = g
                self.acc(x, yv.g)
            self.tape.append(bwd_out)
        return yv

    # ---- whole network ----
    def forward(self, x, timesteps, context, fps):
        c, m = self.c, self.m
        B, Cin, T, H, W_ = x.shape
        mc, te = c.model_channels, 4 * c.model_channels
        dev = self.dev
        # time / fps embedding (openaimodel3d.py:651-660): sinusoid -> Linear -> SiLU -> Linear, summed
        def embed(idx, name):
            sin = self.E(B, mc); ops.timestep_embedding(idx.to(torch.int64).contiguous(), sin, True, 0.0)
            l0 = self.E(B, te); ops.gemm(sin, self.W(name + ".0.weight"), l0, self.W(name + ".0.bias"))
            a0 = self.E(B, te); ops.silu(l0, a0)
            return sin, l0, a0
        sin_t, l0_t, a0_t = embed(timesteps, "time_embed")
        emb = self.E(B, te); ops.gemm(a0_t, self.W("time_embed.2.weight"), emb, self.W("time_embed.2.bias"))
        fcond = c.fps_cond or c.fs_condition
        if fcond:
            sin_f, l0_f, a0_f = embed(fps, "fps_embedding")
            emb2 = self.E(B, te)
            ops.gemm(a0_f, self.W("fps_embedding.2.weight"), emb2, self.W("fps_embedding.2.bias"), epilogue=EPI_GATED_RES, residual=emb)
            emb = emb2
        self.emb = emb                      # time (+ fps / fs) embedding sum [B, te] before SiLU: UNetModel.last_emb
        se = self.E(B, te); ops.silu(emb, se)
        sev = _Var(se)
        demb = torch.zeros(B, te, dtype=F32, device=dev) if self.save else None            # d loss / d SiLU(emb), summed over the ResBlocks
        if self.save and not self.frozen:
            def bwd_emb():
                d_emb = torch.zeros(B, te, dtype=F32, device=dev)
                ops.silu_bwd(demb, emb, d_emb)
                for (sin, l0, a0, name) in ([(sin_t, l0_t, a0_t, "time_embed")] + ([(sin_f, l0_f, a0_f, "fps_embedding")] if fcond else [])):
                    da0 = torch.zeros(B, te, dtype=F32, device=dev)
                    ops.small_linear_bwd(d_emb, a0, self.W(name + ".2.weight"), self.G(name + ".2.weight"), self.G(name + ".2.bias"), da0)
                    dl0 = torch.zeros(B, te, dtype=F32, device=dev)
                    ops.silu_bwd(da0, l0, dl0)
                    ops.small_linear_bwd(dl0, sin, self.W(name + ".0.weight"), self.G(name + ".0.weight"), self.G(name + ".0.bias"), None)
            self.tape.append(bwd_emb)
        # context: the first text_context_len rows of every sample (attention.py:117-118), one [B*L, ctx] operand for all layers
        L = min(context.shape[1], c.text_context_len)
        cdim = context.shape[2]
        ctx2, ctx_ext = self.act(B * L, cdim, True)      # LoRA mode: to_k / to_v of the text cross-attentions are adapted -> extended buffer
        ctx2.copy_(context[:, :L].reshape(B * L, cdim))
        ctxv = _Var(ctx2, ctx_ext, shared=True); ctxv.g = False       # frozen text encoder: no gradient wanted
        # image context (openaimodel3d_dc.py:686-693): 77 + T*16 rows = 16 image tokens for EVERY frame -> B*T items; any other length:
        # the rows after the text are one image set per sample -> B items
        img = None
        self._img_ctx = None
        if c.img_cross_attention:
            Lc, Li = context.shape[1], c.img_context_len
            if Lc <= L:
                raise ValueError(f"img_cross_attention: the context has {Lc} rows, no image tokens after the {L} text tokens")
            NI, Sb = (B * T, Li) if Lc == L + T * Li else (B, Lc - L)
            if Sb > 32:
                raise NotImplementedError(f"img_cross_attention: {Sb} image tokens per item (context of {Lc} rows, {T} frames); "
                                          f"the attention kernel holds up to 32 (csrc/attn_dual.hip)")
            img2 = self.E(NI * Sb, cdim)
            img2.copy_(context[:, L:].reshape(NI * Sb, cdim))
            imgv = _Var(img2)
            if self.save and context.requires_grad:
                imgv.g32 = torch.zeros(NI * Sb, cdim, dtype=F32, device=dev)      # summed over the 16 blocks in fp32
                self._img_ctx = (imgv, B, L, Lc, context.dtype)
            else:
                imgv.g = False
            img = (imgv, NI, Sb)
        # input: [B,C,T,H,W] -> channels-last rows, 4 channels padded to one 64-wide K-tile
        x64 = torch.zeros(B, T, H, W_, 64, dtype=BF16, device=dev)
        x64[..., :Cin] = x.permute(0, 2, 3, 4, 1)
        shape = [B, T, H, W_]
        hs: List = []

        trace = _trace_file()

        def run_layers(layers, h: _Var) -> _Var:
            nonlocal shape
            for l in layers:
                Bq, Tq, Hq, Wq = shape
                if trace is not None:
                    torch.cuda.synchronize()
                    trace.write(f"fwd {l.kind} {l.pre} shape {shape}\n"); trace.flush()
                if l.kind == "conv_in":
                    y5 = self.conv(x64, l.pre + ".weight", l.pre + ".bias", (1, 3, 3), (0, 1, 1), wk=self.P.w["conv_in"])
                    h = _Var(y5.view(-1, l.cout))
                    if self.save:
                        def bwd_in(h=h, l=l):
                            self.conv_bwd(h.g.view(Bq, Tq, Hq, Wq, l.cout), x64, l.pre + ".weight", l.pre + ".bias", (1, 3, 3), (0, 1, 1), 1,
                                          need_dx=False, cin_true=Cin)
                        self.tape.append(bwd_in)
                elif l.kind == "res":
                    h = self.res_block(l, h, shape, sev, demb)
                elif l.kind == "st":
                    h = self.spatial_transformer(l, h, shape, ctxv, L, img)
                elif l.kind == "tt":
                    h = self.temporal_transformer(l, h, shape)
                elif l.kind == "down":
                    xin = h
                    y5 = self.conv(xin.d.view(Bq, Tq, Hq, Wq, l.c), l.pre + ".op.weight", l.pre + ".op.bias", (1, 3, 3), (0, 1, 1), stride=2)
                    h = _Var(y5.view(-1, l.c))
                    shape = [Bq, Tq, y5.shape[2], y5.shape[3]]
                    if self.save:
                        def bwd_dn(h=h, xin=xin, l=l, so=(y5.shape[2], y5.shape[3])):
                            dx5 = self.conv_bwd(h.g.view(Bq, Tq, so[0], so[1], l.c), xin.d.view(Bq, Tq, Hq, Wq, l.c), l.pre + ".op.weight",
                                                l.pre + ".op.bias", (1, 3, 3), (0, 1, 1), 2)
                            self.acc(xin, dx5.view(-1, l.c))
                        self.tape.append(bwd_dn)
                elif l.kind == "up":
                    xin = h
                    up = self.E(Bq * Tq * 4 * Hq * Wq, l.c)
                    ops.row_map(xin.d, up, 1, Bq * Tq, Hq, Wq)
                    y5 = self.conv(up.view(Bq, Tq, 2 * Hq, 2 * Wq, l.c), l.pre + ".conv.weight", l.pre + ".conv.bias", (1, 3, 3), (0, 1, 1))
                    h = _Var(y5.view(-1, l.c))
                    shape = [Bq, Tq, 2 * Hq, 2 * Wq]
                    if self.save:
                        def bwd_up(h=h, xin=xin, l=l, up=up):
                            dup = self.conv_bwd(h.g.view(Bq, Tq, 2 * Hq, 2 * Wq, l.c), up.view(Bq, Tq, 2 * Hq, 2 * Wq, l.c), l.pre + ".conv.weight",
                                                l.pre + ".conv.bias", (1, 3, 3), (0, 1, 1), 1)
                            dx = self.E(Bq * Tq * Hq * Wq, l.c)
                            ops.row_map(dup.view(-1, l.c), dx, 3, Bq * Tq, Hq, Wq)
                            self.acc(xin, dx)
                        self.tape.append(bwd_up)
            return h

        st = m.structure
        h = None
        for i, blk in enumerate(st.input):
            h = run_layers(blk, h)
            if i == 0 and st.init_attn is not None:
                h = run_layers([st.init_attn], h)
            hs.append(h)
        h = run_layers(st.middle, h)
        for blk in st.output:
            skip = hs.pop()
            c1, c2 = h.d.shape[1], skip.d.shape[1]
            cat = self.E(h.d.shape[0], c1 + c2)
            cat[:, :c1].copy_(h.d); cat[:, c1:].copy_(skip.d)            # torch.cat([h, hs.pop()], dim=1): a column concat here
            cv = _Var(cat)
            if self.save:
                def bwd_cat(cv=cv, a=h, b=skip, c1=c1):
                    self.acc(a, cv.g[:, :c1])
                    self.acc(b, cv.g[:, c1:])
                self.tape.append(bwd_cat)
            h = run_layers(blk, cv)
        Bq, Tq, Hq, Wq = shape
        n = self.groupnorm(h, "out.0", Bq * Tq, 1e-5, True)
        y5 = self.conv(n.d.view(Bq, Tq, Hq, Wq, -1), "out.2.weight", "out.2.bias", (1, 3, 3), (0, 1, 1))
        Co = c.out_channels
        if self.save:
            def bwd_out():
                g5 = self._dout5
                n.g = self.conv_bwd(g5, n.d.view(Bq, Tq, Hq, Wq, -1), "out.2.weight", "out.2.bias", (1, 3, 3), (0, 1, 1), 1).view(-1, n.d.shape[1])
            self.tape.append(bwd_out)
        out = y5.permute(0, 4, 1, 2, 3).contiguous()                     # -> [B, C_out, T, H, W] (the reference's layout at the boundary)
        return out, None

    def context_grad(self):
        """d loss / d context after backward(): zeros for the text rows (frozen encoder), the fp32 sum over all blocks for the image rows"""
        if self._img_ctx is None:
            return None
        imgv, B, L, Lc, dt = self._img_ctx
        cdim = imgv.g32.shape[1]
        g = torch.zeros(B, Lc, cdim, dtype=F32, device=self.dev)
        g[:, L:] = imgv.g32.view(B, Lc - L, cdim)
        return g.to(dt)

    def backward(self, dout):
        """dout [B, C_out, T, H, W] bf16"""
        B, Co, T, H, W_ = dout.shape
        g = torch.zeros(B, T, H, W_, (Co + 7) // 8 * 8, dtype=BF16, device=self.dev)
        g[..., :Co] = dout.permute(0, 2, 3, 4, 1)
        self._dout5 = g[..., :Co]
        trace = _trace_file()
        while self.tape:
            fn = self.tape.pop()
            fn()
            if trace is not None:           # VT_UNET_TRACE=<file>: synchronise after every backward closure and log it (fault hunting)
                torch.cuda.synchronize()
                trace.write(f"bwd {len(self.tape)} {fn.__name__}\n"); trace.flush()
        self._dout5 = None
