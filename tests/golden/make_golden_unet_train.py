#!/usr/bin/env python3
"""Golden vectors for the TRAIN-MODE pieces of the VideoCrafter2 path, produced by IMPORTING the reference's own modules (build
container only; stubs as in make_golden_unet.py):

  * TemporalConvBlock under .train(): its three REAL nn.Dropout(0.1) modules run (seeded CPU generator); a forward hook records the keep mask
    each one drew (out != 0), so the fixture holds input, masks, output, input gradient and parameter gradients
    (videotuna/models/lvdm/modules/networks/openaimodel3d.py:258-310);
  * the whole UNetModel under .train() the same way (masks of every TemporalConvBlock, output, loss, gradient checksums);
  * LoRA: peft is absent offline, so the adapters are injected by hand with peft's Linear formula y = W x + (lora_alpha / r) B(A x) on the
    modules the recipe targets (configs/001_videocrafter2/vc2_t2v_lora.yaml:7-12: to_q / to_k / to_v; videotuna/models/lvdm/ddpm3d.py:100-117,
    434-445) -- every CrossAttention of the reference UNetModel; base weights frozen; output, loss and every adapter gradient.

    python tests/golden/make_golden_unet_train.py   -> tests/golden/unet_train.part*.npz
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
import golden_io  # noqa: E402  (fixtures of more than 1 MiB are stored in parts)
import make_golden as MG  # noqa: E402
import unet_oracle as U   # noqa: E402


class LoraLinearByHand(nn.Module):
    """peft.tuners.lora.Linear.forward with lora_dropout = 0: result = base(x) + lora_B(lora_A(x)) * scaling"""

    def __init__(self, base: nn.Linear, a: torch.Tensor, b: torch.Tensor, scaling: float):
        super().__init__()
        self.base_layer = base
        self.lora_A = nn.ModuleDict({"default": nn.Linear(a.shape[1], a.shape[0], bias=False)})
        self.lora_B = nn.ModuleDict({"default": nn.Linear(b.shape[1], b.shape[0], bias=False)})
        with torch.no_grad():
            self.lora_A["default"].weight.copy_(a); self.lora_B["default"].weight.copy_(b)
        self.scaling = scaling

    def forward(self, x):
        return self.base_layer(x) + self.lora_B["default"](self.lora_A["default"](x)) * self.scaling


def hook_masks(module, masks, prefix):
    """record the keep mask of every nn.Dropout below `module` under '<prefix><path of its Sequential>' (e.g. ...temopral_conv.conv2)"""
    hs = []
    for name, m in module.named_modules():
        if isinstance(m, nn.Dropout) and m.p > 0:
            key = prefix + name.rsplit(".", 1)[0]
            def fn(mod, inp, out, key=key):
                masks[key] = (out != 0).to(torch.uint8)
                assert abs(masks[key].float().mean().item() - (1 - mod.p)) < 0.05
            hs.append(m.register_forward_hook(fn))
    return hs


def main():
    MG.install_stubs()
    sys.path.insert(0, MG.REF)
    from videotuna.models.lvdm.modules.networks import openaimodel3d as om
    from videotuna.models.lvdm.modules import attention as at
    cfg = U.tiny_config()
    net = om.UNetModel(in_channels=cfg.in_channels, out_channels=cfg.out_channels, model_channels=cfg.model_channels,
                       attention_resolutions=list(cfg.attention_resolutions), num_res_blocks=cfg.num_res_blocks,
                       channel_mult=list(cfg.channel_mult), num_head_channels=cfg.num_head_channels, transformer_depth=1,
                       context_dim=cfg.context_dim, use_linear=True, use_checkpoint=False, temporal_conv=True, temporal_attention=True,
                       temporal_selfatt_only=True, use_relative_position=False, use_causal_attention=False,
                       temporal_length=cfg.temporal_length, addition_attention=True, fps_cond=True)
    P = U.init_params(cfg, seed=11)
    net.load_state_dict(P, strict=True)
    g = torch.Generator().manual_seed(21)
    rec = {}

    # ---------------- TemporalConvBlock, train mode, real nn.Dropout ----------------
    tcb = net.input_blocks[1][0].temopral_conv.train()
    pre = "input_blocks.1.0.temopral_conv."
    masks = {}
    hs = hook_masks(tcb, masks, pre)
    assert len(hs) == 3
    x = torch.randn(2, 64, 4, 8, 8, generator=g).requires_grad_(True)
    torch.manual_seed(1234)
    y = tcb(x)
    gy = torch.randn(y.shape, generator=g)
    (y * gy).sum().backward()
    rec["tconv.x"], rec["tconv.y"], rec["tconv.gy"], rec["tconv.gx"] = x.detach().numpy(), y.detach().numpy(), gy.numpy(), x.grad.numpy()
    for k, m in masks.items():
        rec["tconv.mask." + k] = m.numpy()
    for n, p in tcb.named_parameters():
        rec["tconv.g." + n] = p.grad.detach().numpy()
    for h in hs:
        h.remove()

    # ---------------- whole UNet, train mode ----------------
    net.train()
    for p in net.parameters():
        p.grad = None
    masks = {}
    hs = hook_masks(net, masks, "")
    B, T, H, W = 2, cfg.temporal_length, 8, 8
    xx = torch.randn(B, cfg.in_channels, T, H, W, generator=g)
    ctx = torch.randn(B, 77, cfg.context_dim, generator=g)
    t = torch.tensor([101, 640]); fps = torch.tensor([24, 16])
    noise = torch.randn(xx.shape, generator=g)
    torch.manual_seed(99)
    out = net(xx, t, context=ctx, fps=fps)
    loss = ((out - noise) ** 2).mean(dim=(1, 2, 3, 4)).mean()
    loss.backward()
    rec.update({"net.x": xx.numpy(), "net.context": ctx.numpy(), "net.t": t.numpy(), "net.fps": fps.numpy(), "net.noise": noise.numpy(),
                "net.out": out.detach().numpy(), "net.loss": np.float64(loss.item())})
    names = [n for n, _ in net.named_parameters()]
    rec["net.grad_sum"] = np.array([float(p.grad.double().sum()) for _, p in net.named_parameters()])
    rec["net.grad_abs_sum"] = np.array([float(p.grad.double().abs().sum()) for _, p in net.named_parameters()])
    for k, m in masks.items():
        rec["net.mask." + k] = np.packbits(m.numpy().reshape(-1))          # bit-packed: 1/8 of the bytes
        rec["net.maskshape." + k] = np.array(m.shape)
    print("train-mode UNet: dropout sites", len(masks), "loss", loss.item())
    for h in hs:
        h.remove()

    # ---------------- LoRA by hand on to_q / to_k / to_v of every CrossAttention, base frozen, eval mode (lora_dropout 0) ----------------
    net.eval()
    r, alpha = 4, 1.0
    L = U.init_lora(cfg, r=r, lora_alpha=alpha, seed=3, zero_b=False)
    sites = U.lora_sites(cfg)
    for p in net.parameters():
        p.requires_grad_(False); p.grad = None
    found = 0
    for name, mod in list(net.named_modules()):
        if isinstance(mod, at.CrossAttention):
            for tgt in ("to_q", "to_k", "to_v"):
                full = f"{name}.{tgt}"
                assert full in sites, full
                setattr(mod, tgt, LoraLinearByHand(getattr(mod, tgt), L[full + ".lora_A.default.weight"], L[full + ".lora_B.default.weight"], alpha / r))
                found += 1
    assert found == len(sites), (found, len(sites))
    out = net(xx, t, context=ctx, fps=fps)
    loss = ((out - noise) ** 2).mean(dim=(1, 2, 3, 4)).mean()
    loss.backward()
    rec["lora.out"], rec["lora.loss"] = out.detach().numpy(), np.float64(loss.item())
    rec["lora.r"], rec["lora.alpha"] = np.int64(r), np.float64(alpha)
    lp = {n: p for n, p in net.named_parameters() if "lora_" in n}
    assert len(lp) == 2 * len(sites) and all(p.grad is not None for p in lp.values())
    assert all(p.grad is None for n, p in net.named_parameters() if "lora_" not in n)
    for n, p in lp.items():
        rec["lora.g." + n] = p.grad.detach().numpy()
    print("LoRA UNet: sites", len(sites), "adapter tensors", len(lp), "loss", loss.item())
    parts = golden_io.save(os.path.join(HERE, "unet_train.npz"), **rec)
    print("unet_train.npz:", len(rec), "arrays,", sum(os.path.getsize(p) for p in parts) // 1024, "KiB")


if __name__ == "__main__":
    main()
