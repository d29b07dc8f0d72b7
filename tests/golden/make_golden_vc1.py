#!/usr/bin/env python3
"""Golden vectors for the VideoCrafter1 layout (use_relative_position=True, temporal_conv=False), produced by IMPORTING the reference's
own modules (build container only):
  videotuna/models/lvdm/modules/attention.py               RelativePosition (19-42), CrossAttention's relative_position branch (126-149),
                                                           TemporalTransformer (395-519: both attn1 and attn2 get the tables)
  videotuna/models/lvdm/modules/networks/openaimodel3d.py  UNetModel (313-694)
Stubs as make_golden_unet.py.  The UNet's weights come from tests/relpos_ref.vc1_init_params (seeded; nothing left at zero, tables drawn
randn x 0.25), so the fixtures hold only inputs, outputs, gradients, name lists and the small attention module's seeded weights.

    python tests/golden/make_golden_vc1.py   -> tests/golden/vc1_attn.npz, vc1_unet_tiny.npz (or parts)
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
import relpos_ref as RR   # noqa: E402

KEEP = ["input_blocks.0.0.weight", "time_embed.0.weight", "fps_embedding.2.bias",
        "init_attn.0.transformer_blocks.0.attn1.to_q.weight", "init_attn.0.transformer_blocks.0.attn1.relative_position_v.embeddings_table",
        "input_blocks.1.2.transformer_blocks.0.attn1.relative_position_k.embeddings_table",
        "input_blocks.1.2.transformer_blocks.0.attn1.to_k.weight", "input_blocks.1.2.transformer_blocks.0.ff.net.0.proj.weight",
        "middle_block.2.transformer_blocks.0.attn2.relative_position_v.embeddings_table",
        "middle_block.2.transformer_blocks.0.attn2.to_v.weight", "output_blocks.3.2.transformer_blocks.0.attn2.relative_position_k.embeddings_table",
        "input_blocks.1.1.transformer_blocks.0.attn2.to_k.weight", "output_blocks.1.0.skip_connection.weight", "out.2.weight", "out.0.bias"]
ATTN_CASES = [(16, 16, 5), (8, 4, 6)]          # (T, P, sequences)


def main():
    MG.install_stubs()
    sys.path.insert(0, MG.REF)
    from videotuna.models.lvdm.modules.networks import openaimodel3d as om
    from videotuna.models.lvdm.modules import attention as at
    assert not at.XFORMERS_IS_AVAILBLE

    # ---------------- (a) CrossAttention(relative_position=True) alone, as self-attention ----------------
    g = torch.Generator().manual_seed(41)
    rec = {}
    for T, P, n in ATTN_CASES:
        ca = at.CrossAttention(query_dim=128, heads=2, dim_head=64, relative_position=True, temporal_length=P)
        assert ca.relative_position_k.embeddings_table.shape == (2 * P + 1, 64)
        with torch.no_grad():
            for name, p in ca.named_parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (0.25 if name.endswith("embeddings_table") else (0.1 if p.dim() == 1 else 128 ** -0.5)))
        x = torch.randn(n, T, 128, generator=g).requires_grad_(True)
        y = ca(x)
        gy = torch.randn(y.shape, generator=g)
        (y * gy).sum().backward()
        tag = f"T{T}P{P}."
        rec[tag + "x"], rec[tag + "y"], rec[tag + "gy"], rec[tag + "gx"] = x.detach().numpy(), y.detach().numpy(), gy.numpy(), x.grad.numpy()
        for name, p in ca.named_parameters():
            rec[tag + "w." + name] = p.detach().numpy()
            rec[tag + "g." + name] = p.grad.numpy()
        rec[tag + "names"] = np.array([name for name, _ in ca.named_parameters()])
    golden_io.save(os.path.join(HERE, "vc1_attn.npz"), **rec)
    print("vc1_attn:", len(rec), "arrays")

    # ---------------- (b) the tiny UNet ----------------
    cfg = RR.vc1_tiny_config()
    net = om.UNetModel(in_channels=cfg.in_channels, out_channels=cfg.out_channels, model_channels=cfg.model_channels,
                       attention_resolutions=list(cfg.attention_resolutions), num_res_blocks=cfg.num_res_blocks,
                       channel_mult=list(cfg.channel_mult), num_head_channels=cfg.num_head_channels, transformer_depth=1,
                       context_dim=cfg.context_dim, use_linear=True, use_checkpoint=True, temporal_conv=False, temporal_attention=True,
                       temporal_selfatt_only=True, use_relative_position=True, use_causal_attention=False,
                       temporal_length=cfg.temporal_length, addition_attention=True, fps_cond=True).eval()
    P = RR.vc1_init_params(cfg, seed=17)
    names = [k for k, _ in net.named_parameters()]
    assert list(P) == names, "restatement parameter list / order differs from the reference module"
    net.load_state_dict(P, strict=True)
    g = torch.Generator().manual_seed(7)
    B, T, H, W = 2, cfg.temporal_length, 8, 8
    x = torch.randn(B, cfg.in_channels, T, H, W, generator=g)
    ctx = torch.randn(B, 80, cfg.context_dim, generator=g).requires_grad_(True)
    t = torch.tensor([37, 912])
    fps = torch.tensor([24, 8])
    noise = torch.randn(x.shape, generator=g)
    out = net(x, t, context=ctx, fps=fps)
    loss = ((out - noise) ** 2).mean(dim=(1, 2, 3, 4)).mean()
    loss.backward()
    params = dict(net.named_parameters())
    rec = dict(x=x.numpy(), context=ctx.detach().numpy(), t=t.numpy(), fps=fps.numpy(), noise=noise.numpy(), out=out.detach().numpy(),
               loss=np.float64(loss.item()), grad_context=ctx.grad.numpy(), names=np.array(names),
               grad_sum=np.array([float(params[n].grad.double().sum()) for n in names]),
               grad_abs_sum=np.array([float(params[n].grad.double().abs().sum()) for n in names]))
    for n in KEEP:
        rec["grad." + n] = params[n].grad.detach().numpy()
    golden_io.save(os.path.join(HERE, "vc1_unet_tiny.npz"), **rec)
    print("vc1_unet_tiny: out", tuple(out.shape), "loss", loss.item(), "params", len(names), sum(p.numel() for p in net.parameters()))


if __name__ == "__main__":
    main()
