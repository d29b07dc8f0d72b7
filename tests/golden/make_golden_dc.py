#!/usr/bin/env python3
"""Golden vectors for the DynamiCrafter UNet path, produced by IMPORTING the reference's own modules (build container only):
  videotuna/models/lvdm/modules/networks/openaimodel3d_dc.py  UNetModel (352-735: img_cross_attention, fs_condition, in_channels 8)
  videotuna/models/lvdm/modules/attention.py                  CrossAttention with img_cross_attention (45-170, einsum path: xformers
                                                              is absent), SpatialTransformer
  videotuna/models/lvdm/modules/encoders/ip_resampler.py      Resampler (65-152)
  videotuna/utils/diffusion_utils.py                          rescale_zero_terminal_snr (the recipe's rescale_betas_zero_snr: True)
Stubs as make_golden_unet.py.  Weights come from tests/dc_oracle.dc_init_params (seeded; the reference's zero-initialised layers --
fps_embedding[-1], proj_out, ... -- get random weights so gradients flow), so the fixture holds only inputs, outputs, gradients and
the list of parameter names.  Modules run in eval() mode (dropout is the identity).

    python tests/golden/make_golden_dc.py   -> tests/golden/dc_unet_tiny.npz (or parts), dc_xattn.npz, dc_resampler.npz, dc_masks.npz, dc_schedule.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
import golden_io  # noqa: E402
import make_golden as MG  # noqa: E402
import dc_oracle as DC    # noqa: E402

KEEP = ["input_blocks.0.0.weight", "time_embed.0.weight", "fps_embedding.0.weight", "fps_embedding.2.weight", "fps_embedding.2.bias",
        "input_blocks.1.1.transformer_blocks.0.attn2.to_k.weight", "input_blocks.1.1.transformer_blocks.0.attn2.to_q.weight",
        "input_blocks.1.1.transformer_blocks.0.attn2.to_k_ip.weight", "input_blocks.1.1.transformer_blocks.0.attn2.to_v_ip.weight",
        "middle_block.1.transformer_blocks.0.attn2.to_k_ip.weight", "middle_block.1.transformer_blocks.0.attn2.to_v_ip.weight",
        "output_blocks.3.1.transformer_blocks.0.attn2.to_v_ip.weight", "output_blocks.3.1.transformer_blocks.0.attn2.to_out.0.weight",
        "input_blocks.1.2.transformer_blocks.0.attn2.to_k.weight", "out.2.weight"]


def main():
    MG.install_stubs()
    sys.path.insert(0, MG.REF)
    from videotuna.models.lvdm.modules.networks import openaimodel3d_dc as om
    from videotuna.models.lvdm.modules import attention as at
    assert not at.XFORMERS_IS_AVAILBLE
    cfg = DC.dc_tiny_config()
    net = om.UNetModel(in_channels=cfg.in_channels, out_channels=cfg.out_channels, model_channels=cfg.model_channels,
                       attention_resolutions=list(cfg.attention_resolutions), num_res_blocks=cfg.num_res_blocks,
                       channel_mult=list(cfg.channel_mult), dropout=0.1, num_head_channels=cfg.num_head_channels, transformer_depth=1,
                       context_dim=cfg.context_dim, use_linear=True, use_checkpoint=True, temporal_conv=True, temporal_attention=True,
                       temporal_selfatt_only=True, use_relative_position=False, use_causal_attention=False,
                       temporal_length=cfg.temporal_length, addition_attention=True, img_cross_attention=True, default_fs=10,
                       fs_condition=True).eval()
    P = DC.dc_init_params(cfg, seed=21)
    names = [k for k, _ in net.named_parameters()]
    assert list(P) == names, "restatement parameter list / order differs from the reference module"
    net.load_state_dict(P, strict=True)
    g = torch.Generator().manual_seed(9)
    B, T, H, W = 2, cfg.temporal_length, 8, 8
    x = torch.randn(B, cfg.in_channels, T, H, W, generator=g)
    ctx = torch.randn(B, 77 + T * DC.IMG_TOKENS, cfg.context_dim, generator=g).requires_grad_(True)      # per-frame image tokens
    t = torch.tensor([37, 912])
    fs = torch.tensor([24, 3])
    noise = torch.randn(B, cfg.out_channels, T, H, W, generator=g)
    out = net(x, t, context=ctx, fs=fs)
    loss = ((out - noise) ** 2).mean(dim=(1, 2, 3, 4)).mean()
    loss.backward()
    params = dict(net.named_parameters())
    rec = dict(x=x.numpy(), context=ctx.detach().numpy(), t=t.numpy(), fs=fs.numpy(), noise=noise.numpy(), out=out.detach().numpy(),
               loss=np.float64(loss.item()), grad_context=ctx.grad.numpy(), names=np.array(names),
               grad_sum=np.array([float(params[n].grad.double().sum()) for n in names]),
               grad_abs_sum=np.array([float(params[n].grad.double().abs().sum()) for n in names]))
    assert float(ctx.grad[:, :77].abs().max()) > 0 and float(ctx.grad[:, 77:].abs().max()) > 0
    for n in KEEP:
        rec["grad." + n] = params[n].grad.detach().numpy()
    with torch.no_grad():
        rec["out_default_fs"] = net(x, t, context=ctx.detach()).numpy()                       # fs=None -> default_fs = 10
        ctx_sh = torch.randn(B, 77 + 20, cfg.context_dim, generator=g)                        # not 77 + t*16: one image set for all frames
        rec["context_shared"] = ctx_sh.numpy()
        rec["out_shared"] = net(x, t, context=ctx_sh, fs=fs).numpy()
    golden_io.save(os.path.join(HERE, "dc_unet_tiny.npz"), **rec)
    print("dc_unet_tiny: out", tuple(out.shape), "loss", loss.item(), "params", len(names), sum(p.numel() for p in net.parameters()))

    # ---------------- CrossAttention with the image branch alone ----------------
    ca = net.input_blocks[1][1].transformer_blocks[0].attn2
    assert isinstance(ca, at.CrossAttention) and ca.img_cross_attention and ca.img_cross_attention_scale == 1.0
    for p in ca.parameters():
        p.grad = None
    xa = torch.randn(3, 20, 64, generator=g).requires_grad_(True)
    ca_ctx = torch.randn(3, 77 + 16, 64, generator=g).requires_grad_(True)
    y = ca(xa, ca_ctx)
    gy = torch.randn(y.shape, generator=g)
    (y * gy).sum().backward()
    blk = {"in0": xa.detach().numpy(), "in1": ca_ctx.detach().numpy(), "y": y.detach().numpy(), "gy": gy.numpy(),
           "gin0": xa.grad.numpy(), "gin1": ca_ctx.grad.numpy(), "prefix": np.array("input_blocks.1.1.transformer_blocks.0.attn2")}
    for n, p in ca.named_parameters():
        blk["g." + n] = p.grad.detach().numpy()
    np.savez_compressed(os.path.join(HERE, "dc_xattn.npz"), **blk)
    print("dc_xattn:", len(blk), "arrays")

    # ---------------- Resampler (tiny): output, every parameter gradient ----------------
    from videotuna.models.lvdm.modules.encoders.ip_resampler import Resampler
    rs = Resampler(**DC.RS_TINY).eval()
    RP = DC.rs_init_params(DC.RS_TINY, seed=31)
    assert list(RP) == [k for k, _ in rs.named_parameters()], "Resampler parameter list / order differs from the reference module"
    rs.load_state_dict(RP, strict=True)
    xi = torch.randn(2, 9, DC.RS_TINY["embedding_dim"], generator=g)
    yo = rs(xi)
    gyo = torch.randn(yo.shape, generator=g)
    (yo * gyo).sum().backward()
    rec = {"x": xi.numpy(), "y": yo.detach().numpy(), "gy": gyo.numpy(), "names": np.array(list(RP))}
    for n, p_ in rs.named_parameters():
        rec["g." + n] = p_.grad.detach().numpy()
    golden_io.save(os.path.join(HERE, "dc_resampler.npz"), **rec)
    print("dc_resampler: out", tuple(yo.shape), len(rec), "arrays")

    # ---------------- three-way condition dropout masks (ddpm3d.py:1391-1397, evaluated as written there, uncond_prob 0.05) ----------------
    from einops import rearrange
    uncond_prob = 0.05
    random_num = torch.tensor([0.0, 0.02, 0.049999, 0.05, 0.07, 0.099999, 0.1, 0.12, 0.149999, 0.15, 0.2, 0.5, 0.97, 1.0])
    prompt_mask = rearrange(random_num < 2 * uncond_prob, "n -> n 1 1")
    input_mask = 1 - rearrange((random_num >= uncond_prob).float() * (random_num < 3 * uncond_prob).float(), "n -> n 1 1 1")
    np.savez_compressed(os.path.join(HERE, "dc_masks.npz"), random_num=random_num.numpy(), uncond_prob=np.float64(uncond_prob),
                        prompt_mask=prompt_mask.numpy().reshape(-1), input_mask=input_mask.numpy().reshape(-1))
    print("dc_masks:", prompt_mask.reshape(-1).int().tolist(), input_mask.reshape(-1).int().tolist())

    # ---------------- zero-terminal-SNR schedule of the recipe ----------------
    from videotuna.utils.diffusion_utils import make_beta_schedule, rescale_zero_terminal_snr
    betas = make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.012, cosine_s=8e-3)
    rescaled = rescale_zero_terminal_snr(np.asarray(betas, dtype=np.float64))
    np.savez_compressed(os.path.join(HERE, "dc_schedule.npz"), betas=np.asarray(betas, dtype=np.float64), betas_zero_snr=np.asarray(rescaled, dtype=np.float64),
                        alphas_cumprod_zero_snr=np.cumprod(1.0 - np.asarray(rescaled, dtype=np.float64), axis=0))
    print("dc_schedule: last alphas_cumprod", float(np.cumprod(1.0 - np.asarray(rescaled, dtype=np.float64))[-1]))


if __name__ == "__main__":
    main()
