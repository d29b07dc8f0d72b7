"""VideoCrafter2 UNet on the device (vt355.unet through the C-ABI kernels) against the CPU oracle (oracle/unet_oracle.py, itself
pinned to the imported reference UNetModel by tests/golden/unet_*.npz) -- BASELINE configs[3], SURVEY 8(a) a11-a13, a15."""
import os

import numpy as np
import pytest
import torch

import golden_io
from parity import bf16_leaves, floor_report, overall_bar, poisoned, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _tiny(dev, seed=11, cfg=None):
    import unet_oracle as U
    from vt355.unet import UNetModel
    cfg = cfg or U.tiny_config()
    m = UNetModel(in_channels=cfg.in_channels, out_channels=cfg.out_channels, model_channels=cfg.model_channels,
                  attention_resolutions=list(cfg.attention_resolutions), num_res_blocks=cfg.num_res_blocks,
                  channel_mult=list(cfg.channel_mult), num_head_channels=64, transformer_depth=1, context_dim=cfg.context_dim,
                  use_linear=True, use_checkpoint=True, temporal_conv=True, temporal_attention=True, temporal_selfatt_only=True,
                  use_relative_position=False, use_causal_attention=False, temporal_length=cfg.temporal_length,
                  addition_attention=True, fps_cond=True)
    P = U.init_params(cfg, seed=seed)
    assert list(P) == list(m.state_dict()), "parameter names / order differ from the reference's state_dict"
    m.load_state_dict(P)
    m.to(dev)
    m.eval()            # the reference's fixtures were taken in eval mode; train mode (dropout masks) has its own test below
    Pr = {k: v.detach().float().cpu().double() for k, v in m.state_dict().items()}       # the bf16-rounded weights the device uses
    return U, cfg, m, Pr


def _bf16_grads(U, cfg, Pr, x, t, ctx, fps, noise, masks=None, lora=None):
    """the oracle's train step once more on the CPU in bf16 -- the same rounded weights, inputs, masks and target, every op rounding to bf16,
    the loss accumulated in fp32 from the bf16 output as on the device: {name: gradient} of the base weights and of the adapters in `lora`"""
    Pb = bf16_leaves({**Pr, **(lora or {})})
    out = U.unet_forward(Pb, cfg, x.to(BF), t, ctx.to(BF), fps=fps, dropout_masks=masks)
    assert out.dtype == BF
    U.lvdm_loss(out.float(), noise.float()).backward()
    return {n: v.grad for n, v in Pb.items() if isinstance(v, torch.Tensor)}


def test_tiny_unet_forward_matches_golden_and_oracle(dev):
    """forward on the golden inputs of the REFERENCE UNetModel run (tests/golden/unet_tiny.part*.npz): vs the reference output itself
    (weights differ only by bf16 rounding) and vs the oracle on the rounded weights"""
    U, cfg, m, Pr = _tiny(dev)
    g = golden_io.load("unet_tiny")
    x = torch.from_numpy(g["x"]); ctx = torch.from_numpy(g["context"]); t = torch.from_numpy(g["t"]); fps = torch.from_numpy(g["fps"])
    with torch.no_grad():
        out = m(x.to(dev, BF), t.to(dev), context=ctx.to(dev, BF), fps=fps.to(dev))
    ref = U.unet_forward(Pr, cfg, x.to(BF).double(), t, ctx.to(BF).double(), fps=fps)
    e_or, e_gold = rel_l2(out, ref), rel_l2(out, torch.from_numpy(g["out"]))
    print(f"[unet tiny fwd] rel-L2 vs oracle {e_or:.3e}, vs reference golden (fp32 weights) {e_gold:.3e}")
    assert e_or < 3e-2 and e_gold < 5e-2


def test_tiny_unet_train_step_matches_oracle(dev):
    """eps-MSE loss, every parameter gradient and one AdamW step of the tiny UNet vs the fp64 oracle"""
    from vt355 import ops
    from vt355.optim import FusedAdamW
    U, cfg, m, Pr = _tiny(dev)
    ts = m.enable_training()
    g = golden_io.load("unet_tiny")
    x = torch.from_numpy(g["x"]); ctx = torch.from_numpy(g["context"]); t = torch.from_numpy(g["t"]); fps = torch.from_numpy(g["fps"])
    noise = torch.from_numpy(g["noise"])
    out = m(x.to(dev, BF), t.to(dev), context=ctx.to(dev, BF), fps=fps.to(dev))
    loss = poisoned((1,), torch.float32, dev); dp = poisoned(out.shape, BF, dev)
    ops.mse_loss(out.detach().contiguous(), noise.to(dev), loss, dp)
    out.backward(dp)
    for v in Pr.values():
        v.requires_grad_(True)
    ref = U.unet_forward(Pr, cfg, x.to(BF).double(), t, ctx.to(BF).double(), fps=fps)
    lref = U.lvdm_loss(ref, noise.double())
    lref.backward()
    assert abs(loss.item() - lref.item()) < 2e-2 * lref.item(), (loss.item(), lref.item())
    overall, ofloor, worst, bad, ratio, at = floor_report([(n, m._view(ts.grad, n), Pr[n].grad) for n in m.shapes],
                                                          _bf16_grads(U, cfg, Pr, x, t, ctx, fps, noise), 0.98, 0.2)
    print(f"[unet tiny train] loss dev {loss.item():.6f} oracle {lref.item():.6f}; grads: overall rel-L2 {overall:.3e} (bf16 floor {ofloor:.3e}), "
          f"worst per-parameter {worst:.3e}, worst device / floor {ratio:.2f} at {at}")
    assert not bad, bad[:10]
    assert overall < overall_bar(5e-2, ofloor)
    opt = FusedAdamW(ts.params, lr=1e-3, fullft_state=ts)
    before = ts.flat.clone()
    opt.step()
    assert torch.isfinite(ts.flat).all() and (ts.flat - before).abs().max().item() > 0
    assert torch.equal(ts.flat_bf16.float(), ts.flat.to(BF).float())


def test_tiny_unet_train_mode_dropout_matches_oracle(dev):
    """model.train(): TemporalConvBlock's three nn.Dropout(0.1) per ResBlock (openaimodel3d.py:278-296) are applied by vt_dropout_bf16.  The
    masks are a pure function of (seed, site, element): recomputed here bit for bit by oracle/philox.py from the sites the forward
    recorded and handed to the oracle (itself pinned to the reference's real nn.Dropout run by tests/golden/unet_train.part*.npz); loss and
    every parameter gradient must agree, and must differ from the eval-mode run."""
    import philox
    from vt355 import ops
    U, cfg, m, Pr = _tiny(dev)
    ts = m.enable_training()
    m.train()
    m.dropout_seed = 20240607
    g = golden_io.load("unet_tiny")
    x = torch.from_numpy(g["x"]); ctx = torch.from_numpy(g["context"]); t = torch.from_numpy(g["t"]); fps = torch.from_numpy(g["fps"])
    noise = torch.from_numpy(g["noise"])
    B, _, T, H, W = x.shape
    out = m(x.to(dev, BF), t.to(dev), context=ctx.to(dev, BF), fps=fps.to(dev))
    loss = poisoned((1,), torch.float32, dev); dp = poisoned(out.shape, BF, dev)
    ops.mse_loss(out.detach().contiguous(), noise.to(dev), loss, dp)
    out.backward(dp)
    sites = m.last_dropout_sites
    assert len(sites) == 24 and len({o for _, o, _, _ in sites}) == 24            # 8 ResBlocks x conv2..conv4, distinct counter ranges
    masks = {}
    for name, off, M, C in sites:
        k = philox.dropout_keep_mask(M, C, 0.1, m.dropout_seed, off)               # rows = (b, t, h, w), channels last
        hw = M // (B * T)
        side = int(round(hw ** 0.5))
        masks[name] = torch.from_numpy(k).view(B, T, side, side, C).permute(0, 4, 1, 2, 3)
    for v in Pr.values():
        v.requires_grad_(True)
    ref = U.unet_forward(Pr, cfg, x.to(BF).double(), t, ctx.to(BF).double(), fps=fps, dropout_masks=masks)
    lref = U.lvdm_loss(ref, noise.double())
    lref.backward()
    with torch.no_grad():
        leval = U.lvdm_loss(U.unet_forward(Pr, cfg, x.to(BF).double(), t, ctx.to(BF).double(), fps=fps), noise.double())
    assert abs(lref.item() - leval.item()) > 1e-4 * leval.item()                   # the masks change the result ...
    assert abs(loss.item() - lref.item()) < 2e-2 * lref.item(), (loss.item(), lref.item())
    e_out = rel_l2(out, ref)
    overall, ofloor, worst, bad, ratio, at = floor_report([(n, m._view(ts.grad, n), Pr[n].grad) for n in m.shapes],
                                                          _bf16_grads(U, cfg, Pr, x, t, ctx, fps, noise, masks=masks), 0.98, 0.2)
    print(f"[unet tiny train-mode dropout] loss dev {loss.item():.6f} oracle {lref.item():.6f} (eval {leval.item():.6f}); out rel-L2 {e_out:.3e}; "
          f"grads overall {overall:.3e} (bf16 floor {ofloor:.3e}), worst {worst:.3e}, worst device / floor {ratio:.2f} at {at}")
    assert e_out < 3e-2 and not bad and overall < overall_bar(5e-2, ofloor), bad[:8]
    # a different seed draws different masks; eval mode draws none
    m.dropout_seed = 5
    with torch.no_grad():
        pass
    m.eval()
    out_e = m(x.to(dev, BF), t.to(dev), context=ctx.to(dev, BF), fps=fps.to(dev))
    assert m.last_dropout_sites == [] and rel_l2(out_e, out) > 1e-3


def test_tiny_unet_lora_train_step_matches_oracle(dev):
    """vc2_t2v_lora.yaml's recipe on the tiny UNet: rank-4 adapters on to_q / to_k / to_v of every CrossAttention (K-extension GEMMs), base
    frozen.  Output, eps-MSE loss and all 180 adapter gradients vs the fp64 oracle with the same adapters (oracle/unet_oracle.lora_linear,
    pinned to the REFERENCE UNetModel with hand-injected peft-formula adapters by tests/golden/unet_train.part*.npz); no base-weight gradient
    buffer exists; one fused AdamW step moves only the adapters"""
    from vt355 import ops
    from vt355.optim import FusedAdamW
    U, cfg, m, Pr = _tiny(dev)
    g = golden_io.load("unet_train")
    L = U.init_lora(cfg, r=int(g["lora.r"]), lora_alpha=float(g["lora.alpha"]), seed=3, zero_b=False)
    m.add_lora(int(g["lora.r"]), float(g["lora.alpha"]), ("to_q", "to_k", "to_v"))
    sd = m.state_dict()
    m.load_state_dict({**{k: v for k, v in sd.items() if "lora" not in k}, **{k: v for k, v in L.items() if k != U.LORA_SCALING_KEY}})
    ts = m.enable_lora_training()
    assert m.train_state is None and ts.numel == sum(v.numel() for k, v in L.items() if k != U.LORA_SCALING_KEY)
    Lr = {k: (v.detach().float().cpu().double().requires_grad_(True) if "lora" in k else None) for k, v in m.state_dict().items() if "lora" in k}
    Lr[U.LORA_SCALING_KEY] = L[U.LORA_SCALING_KEY]
    x = torch.from_numpy(g["net.x"]); ctx = torch.from_numpy(g["net.context"]); t = torch.from_numpy(g["net.t"]); fps = torch.from_numpy(g["net.fps"])
    noise = torch.from_numpy(g["net.noise"])
    out = m(x.to(dev, BF), t.to(dev), context=ctx.to(dev, BF), fps=fps.to(dev))
    loss = poisoned((1,), torch.float32, dev); dp = poisoned(out.shape, BF, dev)
    ops.mse_loss(out.detach().contiguous(), noise.to(dev), loss, dp)
    out.backward(dp)
    ref = U.unet_forward({**Pr, **Lr}, cfg, x.to(BF).double(), t, ctx.to(BF).double(), fps=fps)
    lref = U.lvdm_loss(ref, noise.double())
    lref.backward()
    e_out, e_gold = rel_l2(out, ref), rel_l2(out, torch.from_numpy(g["lora.out"]))
    assert abs(loss.item() - lref.item()) < 2e-2 * lref.item(), (loss.item(), lref.item())
    lo = m.lora
    overall, ofloor, worst, bad, ratio, at = floor_report([(n, lo._view(ts.grad, n), Lr[n].grad) for n in lo.shapes],
                                                          _bf16_grads(U, cfg, Pr, x, t, ctx, fps, noise, lora=Lr), 0.98, 0.2)
    print(f"[unet tiny LoRA] out rel-L2 vs oracle {e_out:.3e}, vs reference golden {e_gold:.3e}; loss dev {loss.item():.6f} oracle {lref.item():.6f}; "
          f"adapter grads overall {overall:.3e} (bf16 floor {ofloor:.3e}), worst {worst:.3e} over {len(lo.shapes)} tensors, "
          f"worst device / floor {ratio:.2f} at {at}")
    assert e_out < 3e-2 and e_gold < 5e-2 and not bad and overall < overall_bar(5e-2, ofloor), bad[:8]
    base_before = m.flat_bf16.clone()
    opt = FusedAdamW(ts.params, lr=1e-3, fullft_state=ts)
    before = ts.flat.clone()
    opt.step()
    assert torch.isfinite(ts.flat).all() and (ts.flat - before).abs().max().item() > 0
    assert torch.equal(m.flat_bf16, base_before)                      # the base weights did not move
    # the packed operands follow the optimizer step: a second forward differs
    with torch.no_grad():
        out2 = m(x.to(dev, BF), t.to(dev), context=ctx.to(dev, BF), fps=fps.to(dev))
    assert rel_l2(out2, out) > 1e-5


# ------------------------------------------------------------------------------------------------ each block alone
def _cl(x5):
    """[B, C, T, H, W] -> channels-last rows [B*T*H*W, C]"""
    return x5.permute(0, 2, 3, 4, 1).reshape(-1, x5.shape[1])


def _block_case(dev, kind, full=False):
    """one layer of the tiny UNet through the engine (forward, input gradient, parameter gradients) vs the oracle's function for
    that block -- the oracle functions are pinned to the reference's own blocks by tests/test_oracle_golden.py
    (tests/golden/unet_blocks.part*.npz: ResBlock + TemporalConvBlock, SpatialTransformer, TemporalTransformer, Downsample, Upsample)"""
    from vt355.unet import _Run, _Var
    import unet_oracle as UO
    if full:
        # the shapes of the VideoCrafter2 recipe's first level (configs/001_videocrafter2/vc2_t2v_320x512.yaml: model_channels 320, 5 heads x 64,
        # context 1024, 16 frames of 40 x 64 latents) in a one-level network, so the layers' weights are the only ones allocated
        cfgf = UO.UNetConfig(model_channels=320, channel_mult=(1,), num_res_blocks=1, attention_resolutions=(1,), context_dim=1024, temporal_length=16)
        U, cfg, m, Pr = _tiny(dev, cfg=cfgf)
        Pr = {k: v.float() for k, v in Pr.items()}            # fp32 oracle at this size (the fp64 score tensors of 16 x 5 x 2560^2 would not fit)
    else:
        U, cfg, m, Pr = _tiny(dev)
    ts = m.enable_training()
    st = m.structure
    g = torch.Generator().manual_seed(hash(kind) % 1000)
    B, T, H, W = 2, 4, 8, 8
    if full:
        B, T, H, W = (1 if kind == "st" else 2), 16, 40, 64
        layer = {"res_same": st.input[1][0], "st": st.input[1][1], "tt": st.input[1][2]}[kind]
    else:
        layer = {"res": st.input[3][0], "res_same": st.input[1][0], "st": st.input[1][1], "tt": st.input[1][2], "init_tt": st.init_attn,
                 "down": st.input[2][0], "up": st.output[1][3]}[kind]
    if kind in ("res", "up") and not full:
        H, W = 4, 4
    cin = getattr(layer, "cin", None) or layer.c
    x = (torch.randn(B, cin, T, H, W, generator=g)).to(BF).float()
    emb = torch.randn(B, 4 * cfg.model_channels, generator=g).to(BF).float()
    ctx = torch.randn(B, 77, cfg.context_dim, generator=g).to(BF).float()
    run = _Run(m, save=True)
    xv = _Var(_cl(x).to(dev, BF).contiguous())
    shape = [B, T, H, W]
    for v in Pr.values():
        v.requires_grad_(True)
    dt_ = torch.float32 if full else torch.float64
    se = torch.nn.functional.silu(emb)

    def oracle(Pd, dt):
        """the block's oracle function on the parameters Pd in dtype dt -> (input leaf, embedding leaf or None, output [B, C, T, H, W])"""
        xr = x.to(dt).requires_grad_(True)
        x4 = xr.permute(0, 2, 1, 3, 4).reshape(B * T, cin, H, W)
        er = None
        if kind in ("res", "res_same"):
            # the oracle applies SiLU itself: feed it the pre-activation whose SiLU is `se` rounded to bf16 -> pass se through a patched call
            er = se.to(BF).to(dt).repeat_interleave(T, dim=0).requires_grad_(True)
            import torch.nn.functional as F
            real_silu = F.silu
            try:
                F.silu = lambda t, *a, **k: t if t is er else real_silu(t, *a, **k)
                ref4 = U.res_block(x4, er, Pd, layer.pre, B, True)
            finally:
                F.silu = real_silu
        elif kind == "st":
            ref4 = U.spatial_transformer(x4, ctx.to(dt).repeat_interleave(T, dim=0), Pd, layer.pre, layer.heads)
        else:
            return xr, er, U.temporal_transformer(xr, Pd, layer.pre, layer.heads)
        return xr, er, ref4.reshape(B, T, ref4.shape[1], ref4.shape[2], ref4.shape[3]).permute(0, 2, 1, 3, 4)

    if kind in ("res", "res_same"):
        sev = _Var(se.to(dev, BF)); demb = torch.zeros(B, emb.shape[1], device=dev)
        yv = run.res_block(layer, xv, shape, sev, demb)
    elif kind == "st":
        ctxv = _Var(ctx.to(dev, BF).view(B * 77, -1).contiguous()); ctxv.g = False
        yv = run.spatial_transformer(layer, xv, shape, ctxv, 77)
    elif kind in ("tt", "init_tt"):
        yv = run.temporal_transformer(layer, xv, shape)
    else:
        pytest.skip("down / up run inside forward(): covered by the whole-network test")
    xr, er, ref5 = oracle(Pr, dt_)
    gy = torch.randn(ref5.shape, generator=g).to(BF).float()
    (ref5 * gy.to(dt_)).sum().backward()
    e_out = rel_l2(yv.d, _cl(ref5))
    yv.g = _cl(gy).to(dev, BF).contiguous()
    while run.tape:
        run.tape.pop()()
    e_dx = rel_l2(xv.g, _cl(xr.grad))
    names = [n for n in m.shapes if n.startswith(layer.pre + ".")]
    Pb = bf16_leaves({n: Pr[n] for n in Pr if n.startswith(layer.pre + ".")})           # (at full size too: the bf16 run costs less than the fp32 one)
    _, _, refb = oracle(Pb, BF)
    assert refb.dtype == BF
    (refb.float() * gy).sum().backward()                 # the upstream gradient meets the bf16 output in fp32, as the device's first backward kernel reads it
    _, _, worst, bad, ratio, at = floor_report([(n, m._view(ts.grad, n), Pr[n].grad) for n in names], {n: Pb[n].grad for n in names}, -1.0, 6e-2)
    note = f", worst device / floor {ratio:.2f} at {at}"
    print(f"[unet block {kind}{' FULL SIZE ' + str([B, T, H, W, cin]) if full else ''}] out rel-L2 {e_out:.3e}, dx {e_dx:.3e}, worst parameter gradient {worst:.3e} over {len(names)} tensors{note}")
    assert e_out < 2e-2 and e_dx < 4e-2 and not bad, bad[:8]
    if kind in ("res", "res_same"):
        dse = er.grad.view(B, T, -1).sum(1)
        assert rel_l2(demb, dse) < 4e-2


@pytest.mark.parametrize("kind", ["res", "res_same", "st", "tt", "init_tt"])
def test_unet_block_alone(dev, kind):
    _block_case(dev, kind)


@pytest.mark.parametrize("kind", ["res_same", "st", "tt"])
def test_unet_level0_blocks_at_the_recipes_full_size(dev, kind):
    """BASELINE configs[3] at its stated shapes: one ResBlock (+ TemporalConvBlock), one SpatialTransformer and one TemporalTransformer of the
    first UNet level -- 320 channels, 5 heads x 64, 16 frames of 40 x 64 latents, 77 x 1024 text context -- through the engine against the
    fp32 oracle functions (pinned to the reference's own blocks by tests/golden/unet_blocks.part*.npz): output, input gradient and every parameter
    gradient of the layer.  (Batch 2; the SpatialTransformer at batch 1: the oracle's 16 x 5 x 2560 x 2560 score tensors.)"""
    _block_case(dev, kind, full=True)


def test_whole_unet_full_size_backward_predicts_its_own_forward(dev):
    """BASELINE configs[3] at its stated size, ONE sample: the whole 1.41 B-parameter VideoCrafter2 UNet (320 channels, mult 1-2-4-4, 16 spatial +
    16 temporal transformers) forward + backward on latents [1, 4, 16, 40, 64] with a 77 x 1024 context -- the size no CPU oracle reaches in a
    test's time.  Property checked instead: the gradient the backward returns predicts what the forward does.  For each of six parameter
    groups (convolutions, temporal convolutions, spatial / temporal attention, feed-forward, norms + embeddings + biases) the weights a random subset
    of the weights is moved along that group's own gradient by a few bf16 ulps and  L(w+) - L(w-)  is compared with  <g, w+ - w->  (w+- = the bf16 weights actually
    used: rounding is in the prediction).  A wrong kernel at any full-size shape -- a ragged tile, a descriptor extent, a split that drops
    rows -- breaks the match of its group.  Eval mode (no dropout): the forward must be a function of the weights."""
    from vt355.unet import UNetModel
    m = UNetModel(in_channels=4, out_channels=4, model_channels=320, attention_resolutions=[4, 2, 1], num_res_blocks=2, channel_mult=[1, 2, 4, 4],
                  num_head_channels=64, transformer_depth=1, context_dim=1024, use_linear=True, use_checkpoint=True, temporal_conv=True,
                  temporal_attention=True, temporal_selfatt_only=True, use_relative_position=False, use_causal_attention=False,
                  temporal_length=16, addition_attention=True, fps_cond=True)
    m.init_weights(77)
    m.to(dev)
    m.eval()
    ts = m.enable_training()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 4, 16, 40, 64, generator=g).to(dev, BF)
    ctx = torch.randn(1, 77, 1024, generator=g).to(dev, BF)
    t = torch.tensor([417], device=dev); fps = torch.tensor([24], device=dev)
    r = torch.randn(1, 4, 16, 40, 64, generator=g).to(dev)

    def L():
        with torch.no_grad():
            return (m(x, t, context=ctx, fps=fps).float() * r).sum().item() / r.numel()

    out = m(x, t, context=ctx, fps=fps)
    assert torch.isfinite(out).all()
    out.backward((r / r.numel()).to(BF))
    torch.cuda.synchronize()
    grad = ts.grad.clone()
    assert torch.isfinite(grad).all()
    groups = {"conv": [], "tconv": [], "attn_spatial": [], "attn_temporal": [], "ff": [], "rest": []}
    for n, shp in m.shapes.items():
        if "temopral_conv" in n or "temporal_conv" in n:
            k = "tconv" if len(shp) > 1 else "rest"
        elif ".ff." in n and len(shp) > 1:
            k = "ff"
        elif (".attn1." in n or ".attn2." in n) and len(shp) > 1:
            k = "attn_temporal" if ".2.transformer_blocks" in n or "init_attn" in n else "attn_spatial"
        elif len(shp) >= 4:
            k = "conv"
        else:
            k = "rest"
        groups[k].append(n)
    assert all(groups.values()), {k: len(v) for k, v in groups.items()}
    base_bf16 = ts.flat_bf16.clone()
    dgen = torch.Generator(device=dev).manual_seed(5)
    L0 = L()
    report = []
    for k, names in groups.items():
        d = torch.zeros_like(grad)
        for n in names:
            gv = m._view(grad, n); wv = m._view(ts.flat, n)
            gn = gv.float().pow(2).mean().sqrt()
            if gn > 0:
                m._view(d, n).copy_(gv * (wv.float().pow(2).mean().sqrt() / gn))          # along the gradient, one weight-rms long per tensor
        # the function saturates within a fraction of a percent of weight change along its own gradient, and bf16 weights cannot move by less than
        # an ulp (0.4 - 0.8 %): move only a random SUBSET of the elements, each by 3 % of its tensor's rms, the subset sized for a predicted
        # change of 2e-3 (L itself is ~1e-3 .. 1e-2; the forward's own rounding noise is ~1e-5)
        eps = 0.03
        pred_full = eps * (grad.double() * d.double()).sum().item()
        rho = min(1.0, 2e-3 / max(pred_full, 1e-30))
        mask = torch.rand(d.shape, device=d.device, generator=dgen) < rho
        d = d * mask
        vals = {}
        for sgn in (+1, -1):
            ts.flat_bf16.copy_((ts.flat + sgn * eps * d).to(BF))
            ts.version += 1
            vals[sgn] = (L(), ts.flat_bf16.float().clone())
        ts.flat_bf16.copy_(base_bf16); ts.version += 1
        measured = vals[+1][0] - vals[-1][0]
        predicted = (grad.double() * (vals[+1][1] - vals[-1][1]).double()).sum().item()
        report.append((k, len(names), measured, predicted))
    print(f"[unet full size] L0 {L0:.5e}; " + "; ".join(f"{k} ({n} tensors): dL {a:.4e} vs <g, dw> {b:.4e}" for k, n, a, b in report))
    for k, n, a, b in report:
        assert b > 0 and abs(a - b) <= 0.1 * b, (k, a, b)
