"""fp32 CPU restatement (test infrastructure, NOT product code) of the CogVideoX VAE DECODER the reference holds in-tree:
``SpatialNorm3D`` (cp_enc_dec.py:462-539), ``Upsample3D`` (:560-622), the decoder's ResNet block (:681-777 with ``Normalize3D``) and
``ContextParallelDecoder3D.forward`` (:908-1067), context-parallel world 1 / rank 0 / fake_cp (the first frame handled apart).

The nearest interpolations are written with ``F.interpolate`` as the twin writes them, NOT with the integer index rule of the kernels, so a
wrong rule in ``vt_spatialnorm_silu_cl`` / ``vt_upsample_conv2d_cl`` cannot be shared.  Pinned to the twin by
tests/golden/vae_decoder_tiny / vae_upsample3d / vae_spatialnorm3d (tests/golden/make_golden_vae_decoder.py, tests/test_vae_decoder_cpu.py).

``store_dtype=torch.bfloat16`` rounds every tensor the device path stores (the latent, the modulation tables at latent resolution, every
kernel's output): the run is then one sample of the rounding noise a correct bf16 implementation carries.
``mutant=`` restates the wrong kernels a reviewer would fear (MUTANTS); tests/test_vae_decoder_cpu.py shows that the GPU tests' inputs
separate each of them from the right one.  The inputs of the GPU tests are built here (``*_cases`` / ``*_inputs``) so that both files use
exactly the same ones."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

MUTANTS = ("zq_first", "up_first", "no_conv_b", "no_beta", "mod_before_affine", "hz_off", "no_pad_rb")
SPN_MUTANTS = ("zq_first", "no_conv_b", "no_beta", "mod_before_affine", "hz_off")      # wrong vt_spatialnorm_silu_cl kernels
UP_MUTANTS = ("up_first", "no_pad_rb")                                                 # wrong vt_upsample_conv2d_cl kernels


@dataclass
class VaeDecConfig:
    ch: int = 128
    ch_mult: Tuple[int, ...] = (1, 2, 2, 4)
    num_res_blocks: int = 3
    out_ch: int = 3
    z_channels: int = 16
    temporal_compress_times: int = 4


def tiny_config(**kw) -> VaeDecConfig:
    base = dict(ch=32, ch_mult=(1, 2, 2), num_res_blocks=1, z_channels=4, temporal_compress_times=4)
    base.update(kw)
    return VaeDecConfig(**base)


def swish(x):
    return x * torch.sigmoid(x)


def _st(x, store_dtype):
    return x if store_dtype is None else x.to(store_dtype).to(x.dtype)


def causal_conv3d(x, w, b):
    """x [B, C, T, H, W]; kernel (kt, k, k): kt - 1 copies of the first frame in front of t, zeros around h / w"""
    kt, ks = w.shape[2], w.shape[3]
    if kt > 1:
        x = torch.cat([x[:, :, :1]] * (kt - 1) + [x], dim=2)
    if ks > 1:
        x = F.pad(x, (ks // 2,) * 4)
    return F.conv3d(x, w, b)


def interp_zq(zq, size, mutant=None):
    """SpatialNorm3D.forward's interpolation of the latent to ``size`` = (T, H, W): T > 1 -> first frame apart (:507-523)"""
    T = size[0]
    if T > 1 and mutant != "zq_first":
        first = F.interpolate(zq[:, :, :1], size=(1,) + tuple(size[1:]), mode="nearest")
        rest = F.interpolate(zq[:, :, 1:], size=(T - 1,) + tuple(size[1:]), mode="nearest")
        up = torch.cat([first, rest], dim=2)
    else:
        up = F.interpolate(zq, size=tuple(size), mode="nearest")
    if mutant == "hz_off":                 # hz = (h + 1) // ratio: wrong exactly at the first line of every block but the last
        H = size[1]
        up = up[:, :, :, [min(h + 1, H - 1) for h in range(H)]]
    return up


def _modulate(f, Y, Bm, gamma, beta, silu, mutant):
    if mutant == "mod_before_affine":
        out = (F.group_norm(f, 32, None, None, 1e-6) * Y + Bm) * gamma.view(1, -1, 1, 1, 1) + beta.view(1, -1, 1, 1, 1)
    else:
        nf = F.group_norm(f, 32, gamma, None if mutant == "no_beta" else beta, 1e-6)
        out = nf * Y if mutant == "no_conv_b" else nf * Y + Bm
    return swish(out) if silu else out


def spatial_norm3d(f, zq, gamma, beta, wy, by, wb, bb, silu=False, store_dtype=None, mutant=None):
    """f [B, C, T, H, W], zq [B, Z, Tz, Hz, Wz] -> GroupNorm(f) * conv_y(zq^) + conv_b(zq^) (+ SiLU), the twin's order: interpolate, then the
    1x1x1 convolutions.  store_dtype rounds conv_y / conv_b's outputs (the device stores them, at latent resolution: rounding commutes with
    the nearest interpolation) and the result."""
    zu = interp_zq(zq, f.shape[-3:], mutant)
    Y, Bm = _st(causal_conv3d(zu, wy, by), store_dtype), _st(causal_conv3d(zu, wb, bb), store_dtype)
    return _st(_modulate(f, Y, Bm, gamma, beta, silu, mutant), store_dtype)


def spatial_norm3d_table(f, mod_y, mod_b, gamma, beta, silu=False, mutant=None):
    """the same with conv_y(zq) / conv_b(zq) given at latent resolution [B, C, Tz, Hz, Wz] (what vt_spatialnorm_silu_cl is handed).  Returns
    (out, bar) with bar = 2^-7 (|nf Y| + |B|) per element"""
    Y, Bm = interp_zq(mod_y, f.shape[-3:], mutant), interp_zq(mod_b, f.shape[-3:], mutant)
    out = _modulate(f, Y, Bm, gamma, beta, silu, mutant)
    nf = F.group_norm(f, 32, gamma, beta, 1e-6)
    return out, 2.0 ** -7 * ((nf * Y).abs() + Bm.abs())


def _interp32(x, **kw):
    """F.interpolate per 32-channel split, as the twin does it"""
    return torch.cat([F.interpolate(s, mode="nearest", **kw) for s in torch.split(x, 32, dim=1)], dim=1)


def upsample_nearest(x, compress_time, mutant=None):
    """the interpolation of Upsample3D.forward (:575-615), x [B, C, T, H, W]"""
    B, C, T, H, W = x.shape
    if compress_time and T > 1:
        if mutant == "up_first":           # ts(t) = t // 2 over the same 2T - 1 output frames: the first frame is doubled like the others
            return _interp32(x, scale_factor=2.0)[:, :, :2 * T - 1]
        first = F.interpolate(x[:, :, 0], scale_factor=2.0, mode="nearest")
        rest = _interp32(x[:, :, 1:], scale_factor=2.0)
        return torch.cat([first[:, :, None], rest], dim=2)
    x2 = _interp32(x.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W), scale_factor=2.0)
    return x2.reshape(B, T, C, 2 * H, 2 * W).permute(0, 2, 1, 3, 4)


def upsample3d(x, w, b, compress_time, store_dtype=None, mutant=None):
    """Upsample3D.forward: nearest upsample, then Conv2d(3, padding 1) per frame"""
    u = upsample_nearest(x, compress_time, mutant)
    B, C, T, H, W = u.shape
    u2 = u.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W)
    if mutant == "no_pad_rb":              # reads past the right / bottom edge land on the last line / column instead of zero
        u2 = F.pad(F.pad(u2, (0, 1, 0, 1), mode="replicate"), (1, 0, 1, 0))
        y = F.conv2d(u2, w, b)
    else:
        y = F.conv2d(u2, w, b, padding=1)
    return _st(y.reshape(B, T, -1, H, W).permute(0, 2, 1, 3, 4), store_dtype)


def upsample3d_bar(x, w, compress_time, ref):
    """2^-8 |ref| + 2^-16 conv(|x|, |w|): the output rounding plus fp32 accumulation over 9 Cin terms"""
    return 2.0 ** -8 * ref.abs() + 2.0 ** -16 * upsample3d(x.abs(), w.abs(), None, compress_time)


def resnet_block(x, zq, P, pre, cin, cout, store_dtype=None, mutant=None):
    def sn(h, name):
        q = pre + name
        return spatial_norm3d(h, zq, P[q + ".norm_layer.weight"], P[q + ".norm_layer.bias"], P[q + ".conv_y.conv.weight"],
                              P[q + ".conv_y.conv.bias"], P[q + ".conv_b.conv.weight"], P[q + ".conv_b.conv.bias"], True, store_dtype, mutant)
    h = _st(causal_conv3d(sn(x, "norm1"), P[pre + "conv1.conv.weight"], P[pre + "conv1.conv.bias"]), store_dtype)
    h = causal_conv3d(sn(h, "norm2"), P[pre + "conv2.conv.weight"], P[pre + "conv2.conv.bias"])
    if cin != cout:
        x = _st(F.conv3d(x, P[pre + "nin_shortcut.weight"], P[pre + "nin_shortcut.bias"]), store_dtype)
    return _st(x + h, store_dtype)           # the device adds the skip in the convolution's fp32 epilogue: one rounding


def block_channels(cfg: VaeDecConfig):
    """[(level, [(cin, cout) per block])] in the order the decoder walks them (highest level first)"""
    out, block_in = [], cfg.ch * cfg.ch_mult[-1]
    for i in reversed(range(len(cfg.ch_mult))):
        block_out = cfg.ch * cfg.ch_mult[i]
        out.append((i, [(block_in if j == 0 else block_out, block_out) for j in range(cfg.num_res_blocks + 1)]))
        block_in = block_out
    return out


def init_params(cfg: VaeDecConfig, seed: int = 0, dtype=torch.float32) -> Dict[str, torch.Tensor]:
    """seeded parameters under the twin's names"""
    g = torch.Generator().manual_seed(seed)
    P = {}

    def conv(name, cout, cin, *k):
        P[name + ".weight"] = torch.randn(cout, cin, *k, generator=g) / (cin * math.prod(k)) ** 0.5
        P[name + ".bias"] = 0.1 * torch.randn(cout, generator=g)

    def snorm(name, c):
        P[name + ".norm_layer.weight"] = 1.0 + 0.1 * torch.randn(c, generator=g)
        P[name + ".norm_layer.bias"] = 0.1 * torch.randn(c, generator=g)
        conv(name + ".conv_y.conv", c, cfg.z_channels, 1, 1, 1)
        conv(name + ".conv_b.conv", c, cfg.z_channels, 1, 1, 1)
        P[name + ".conv_y.conv.bias"] += 1.0             # a modulation around 1, as a trained SpatialNorm has

    def block(pre, cin, cout):
        snorm(pre + "norm1", cin); conv(pre + "conv1.conv", cout, cin, 3, 3, 3)
        snorm(pre + "norm2", cout); conv(pre + "conv2.conv", cout, cout, 3, 3, 3)
        if cin != cout:
            conv(pre + "nin_shortcut", cout, cin, 1, 1, 1)

    top = cfg.ch * cfg.ch_mult[-1]
    conv("conv_in.conv", top, cfg.z_channels, 3, 3, 3)
    block("mid.block_1.", top, top); block("mid.block_2.", top, top)
    last = top
    for i, blocks in block_channels(cfg):
        for j, (cin, cout) in enumerate(blocks):
            block(f"up.{i}.block.{j}.", cin, cout)
            last = cout
        if i != 0:
            conv(f"up.{i}.upsample.conv", last, last, 3, 3)
    snorm("norm_out", last)
    conv("conv_out.conv", cfg.out_ch, last, 3, 3, 3)
    return {k: v.to(dtype) for k, v in P.items()}


def decoder_forward(P: Dict[str, torch.Tensor], cfg: VaeDecConfig, z: torch.Tensor, store_dtype=None, mutant: Optional[str] = None) -> torch.Tensor:
    """z [B, z_channels, T', H', W'] -> [B, out_ch, T, H, W]"""
    assert mutant is None or mutant in MUTANTS, mutant
    nlev = len(cfg.ch_mult)
    tlevels = int(math.log2(cfg.temporal_compress_times))
    zq = _st(z, store_dtype)
    h = _st(causal_conv3d(zq, P["conv_in.conv.weight"], P["conv_in.conv.bias"]), store_dtype)
    top = cfg.ch * cfg.ch_mult[-1]
    h = resnet_block(h, zq, P, "mid.block_1.", top, top, store_dtype, mutant)
    h = resnet_block(h, zq, P, "mid.block_2.", top, top, store_dtype, mutant)
    for i, blocks in block_channels(cfg):
        for j, (cin, cout) in enumerate(blocks):
            h = resnet_block(h, zq, P, f"up.{i}.block.{j}.", cin, cout, store_dtype, mutant)
        if i != 0:
            h = upsample3d(h, P[f"up.{i}.upsample.conv.weight"], P[f"up.{i}.upsample.conv.bias"], i >= nlev - tlevels, store_dtype, mutant)
    h = spatial_norm3d(h, zq, P["norm_out.norm_layer.weight"], P["norm_out.norm_layer.bias"], P["norm_out.conv_y.conv.weight"],
                       P["norm_out.conv_y.conv.bias"], P["norm_out.conv_b.conv.weight"], P["norm_out.conv_b.conv.bias"], True, store_dtype, mutant)
    return _st(causal_conv3d(h, P["conv_out.conv.weight"], P["conv_out.conv.bias"]), store_dtype)


def max_norm_err(got, ref):
    """max |got - ref| / max |ref| in fp64"""
    got, ref = got.double(), ref.double()
    return ((got - ref).abs().max() / ref.abs().max()).item()


# ------------------------------------------------------------------ the inputs of the GPU tests (shared with the CPU mutant test)
BF16 = torch.bfloat16


def _r(*shape, g, scale=1.0):
    return (scale * torch.randn(*shape, generator=g)).to(BF16).float()       # bf16-representable fp32


def spn_cases():
    """(C, Tz, T, ratio): C in {64, 128} x (Tz, T) x spatial ratio {1, 2, 8} at (Hz, Wz) = (3, 5), N = 2; every case runs with SiLU on and
    off, on a contiguous and on a strided x (SPN_VARIANTS)"""
    return [(C, Tz, T, ratio) for C in (64, 128) for (Tz, T) in ((1, 1), (2, 3), (2, 5), (3, 3)) for ratio in (1, 2, 8)]


SPN_VARIANTS = ((True, False), (False, False), (True, True), (False, True))        # (silu, strided ldx)


def spn_inputs(case):
    """x [N, C, T, H, W] with a per-channel offset (GroupNorm has a mean to remove), tables around (1, 0), gamma / beta"""
    C, Tz, T, ratio = case
    g = torch.Generator().manual_seed(1000 + C + 10 * Tz + 100 * T + ratio)
    N, Hz, Wz = 2, 3, 5
    x = _r(N, C, T, Hz * ratio, Wz * ratio, g=g) + _r(1, C, 1, 1, 1, g=g, scale=0.5)
    x = x.to(BF16).float()
    mod_y = (1.0 + 0.5 * torch.randn(N, C, Tz, Hz, Wz, generator=g)).to(BF16).float()
    mod_b = _r(N, C, Tz, Hz, Wz, g=g, scale=0.5)
    gamma = (1.0 + 0.2 * torch.randn(C, generator=g)).to(BF16).float()
    beta = _r(C, g=g, scale=0.3)
    return dict(x=x, mod_y=mod_y, mod_b=mod_b, gamma=gamma, beta=beta)


def up_cases():
    """(C, T, temporal): Cin = Cout in {64, 128}, T in {1, 2, 3}, temporal upsampling on and off; N = 2, H x W = 5 x 7"""
    return [(C, T, tup) for C in (64, 128) for T in (1, 2, 3) for tup in (False, True)]


def up_inputs(case):
    C, T, tup = case
    g = torch.Generator().manual_seed(2000 + C + 10 * T + int(tup))
    x = _r(2, C, T, 5, 7, g=g)
    w = _r(C, C, 3, 3, g=g, scale=1.0 / (9 * C) ** 0.5)
    b = _r(C, g=g, scale=0.1)
    return dict(x=x, w=w, b=b, temporal=tup)


DEC_CFG = VaeDecConfig(ch=64, ch_mult=(1, 2, 2), num_res_blocks=1, z_channels=4, temporal_compress_times=4)
DEC_SHAPES = ((3, 2, 3), (1, 2, 3), (2, 3, 2))            # latent (T', H', W'), B = 2


def decoder_inputs(shape, seed=11):          # of the seeds 7 .. 12 the one that leaves the nearest mutant farthest from the bar (17 x it)
    """(P bf16-representable fp32 under the twin's names, z [2, 4, T', H', W']).  The GroupNorm betas are 5 x init_params' (std 0.5, the
    size of the conv_b term): with betas of 0.1 a kernel that drops beta stays within 7 x the test's bar, too close to call"""
    P = {k: ((5.0 * v) if k.endswith("norm_layer.bias") else v).to(BF16).float() for k, v in init_params(DEC_CFG, seed=seed).items()}
    g = torch.Generator().manual_seed(3000 + 100 * shape[0] + 10 * shape[1] + shape[2])
    return P, _r(2, DEC_CFG.z_channels, *shape, g=g)


def make_workflow_dir(tmp_path, with_decoder, vcfg=None):
    """a local HF-layout checkpoint directory of tiny dimensions under tmp_path (DiT, scheduler, VAE in the in-tree twin's names: the encoder's
    own keys, or with_decoder a whole autoencoder file with `encoder.` / `decoder.` sub-trees); returns the workflow's config node, whose
    paths are relative to tmp_path as the reference's YAMLs are to its working directory"""
    import json
    from safetensors.torch import save_file
    from vt355.dit import CogVideoXTransformer3DModel
    from vt355.vae import CogVideoXVaeDecoder, CogVideoXVaeEncoder
    root = "checkpoints/cogvideo/CogVideoX-2b"
    ck = tmp_path / root
    tcfg = dict(num_attention_heads=1, attention_head_dim=64, num_layers=1, time_embed_dim=64, text_embed_dim=64, in_channels=16,
                out_channels=16, sample_width=8, sample_height=4, sample_frames=5, max_text_seq_length=4)
    (ck / "transformer").mkdir(parents=True); (ck / "scheduler").mkdir(); (ck / "vae").mkdir()
    tiny = CogVideoXTransformer3DModel(**tcfg).init_weights(3)
    (ck / "transformer" / "config.json").write_text(json.dumps(tcfg))
    save_file({k: v.contiguous() for k, v in tiny.state_dict().items()}, str(ck / "transformer" / "diffusion_pytorch_model.safetensors"))
    (ck / "scheduler" / "scheduler_config.json").write_text(json.dumps(
        {"_class_name": "CogVideoXDPMScheduler", "num_train_timesteps": 1000, "beta_start": 0.00085, "beta_end": 0.012, "snr_shift_scale": 3.0}))
    vcfg = vcfg or dict(ch=64, ch_mult=[1, 2], num_res_blocks=1, z_channels=16, temporal_compress_times=2, scaling_factor=0.7)
    sd = {k: v.contiguous() for k, v in CogVideoXVaeEncoder(**vcfg).init_weights(1).state_dict().items()}
    if with_decoder:
        sd = {"encoder." + k: v for k, v in sd.items()}
        sd.update({"decoder." + k: v.contiguous() for k, v in CogVideoXVaeDecoder(**vcfg).init_weights(2).state_dict().items()})
    (ck / "vae" / "config.json").write_text(json.dumps(vcfg))
    save_file(sd, str(ck / "vae" / "diffusion_pytorch_model.safetensors"))
    return {"target": "videotuna.models.cogvideo_hf.cogvideo_pl.CogVideoXWorkFlow", "params": {
        "first_stage_config": {"target": "diffusers.AutoencoderKLCogVideoX", "params": {"pretrained_model_name_or_path": root, "subfolder": "vae"}},
        "denoiser_config": {"target": "diffusers.CogVideoXTransformer3DModel", "params": {"pretrained_model_name_or_path": root, "subfolder": "transformer"}},
        "scheduler_config": {"target": "diffusers.CogVideoXDPMScheduler", "params": {"pretrained_model_name_or_path": root, "subfolder": "scheduler"}}}}
