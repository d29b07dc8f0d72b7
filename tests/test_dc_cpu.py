"""CPU checks of the DynamiCrafter path that need no GPU."""
import pytest
import torch

from dc_oracle import dual_attention_autograd, dual_attention_ref


@pytest.mark.parametrize("B,T,HW,H,Sa,Sb,c", [(2, 3, 33, 2, 77, 16, 1.0), (1, 2, 40, 1, 20, 5, 0.5)])
def test_dual_attention_restatement_backward_equals_autograd(B, T, HW, H, Sa, Sb, c):
    """the hand-written float64 backward the GPU tests compare against IS the derivative of the two-softmax formula"""
    g = torch.Generator().manual_seed(HW)
    D = H * 64
    q, do = torch.randn(B, T * HW, D, generator=g), torch.randn(B, T * HW, D, generator=g)
    k, v = torch.randn(B, Sa, D, generator=g), torch.randn(B, Sa, D, generator=g)
    ki, vi = torch.randn(B * T, Sb, D, generator=g), torch.randn(B * T, Sb, D, generator=g)
    ref = dual_attention_ref(q, k, v, ki, vi, H, HW, c, 0.125, do)
    ag = dual_attention_autograd(q, k, v, ki, vi, H, HW, c, do)
    for n in ag:
        assert torch.allclose(ref[n], ag[n], rtol=1e-10, atol=1e-12), n
    # the wrong variants differ from it by far more than any kernel tolerance
    for variant in ("joint_softmax", "frame0_image", "delta_from_o"):
        bad = dual_attention_ref(q, k, v, ki, vi, H, HW, c, 0.125, do, variant)
        worst = max(((bad[n] - ref[n]).abs().max() / ref[n].abs().max()).item() for n in ag)
        assert worst > 0.1, (variant, worst)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement of the DynamiCrafter UNet against the reference's own modules (tests/golden/make_golden_dc.py)
# ---------------------------------------------------------------------------------------------------------------------
import os  # noqa: E402

import numpy as np  # noqa: E402

import dc_oracle as DC  # noqa: E402
import golden_io  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dc_params(dtype=torch.float64):
    cfg = DC.dc_tiny_config()
    return cfg, DC.dc_init_params(cfg, seed=21, dtype=dtype)


def test_dc_unet_restatement_matches_reference_unet():
    """tests/dc_oracle.dc_unet_forward vs openaimodel3d_dc.UNetModel: output, loss, checksums of ALL parameter gradients, 15 gradients
    in full and the gradient of the context (text rows and per-frame image rows) -- the bars of test_oracle_golden.py's UNet test"""
    cfg, P = _dc_params()
    g = golden_io.load("dc_unet_tiny")
    for v in P.values():
        v.requires_grad_(True)
    T = lambda k: torch.from_numpy(g[k])
    ctx = T("context").double().requires_grad_(True)
    out = DC.dc_unet_forward(P, cfg, T("x").double(), T("t"), ctx, fs=T("fs"))
    ref = T("out").double()
    assert (out - ref).abs().max().item() < 2e-5 * ref.abs().max().item()
    loss = ((out - T("noise").double()) ** 2).mean(dim=(1, 2, 3, 4)).mean()
    assert abs(loss.item() - float(g["loss"])) < 1e-5 * float(g["loss"])
    loss.backward()
    names = list(P)
    gs = np.array([P[n].grad.sum().item() for n in names]); ga = np.array([P[n].grad.abs().sum().item() for n in names])
    assert np.allclose(ga, g["grad_abs_sum"], rtol=2e-4, atol=1e-7), np.abs(ga - g["grad_abs_sum"]).max()
    assert np.allclose(gs, g["grad_sum"], rtol=0, atol=2e-4 * np.abs(g["grad_abs_sum"]).max())
    full = [k[5:] for k in g.files if k.startswith("grad.")]
    assert len(full) == 15 and sum("_ip." in n for n in full) == 5
    for n in full:
        r = torch.from_numpy(g["grad." + n]).double()
        assert (P[n].grad - r).abs().max().item() < 2e-4 * r.abs().max().item() + 1e-9, n
    r = T("grad_context").double()
    assert (ctx.grad - r).abs().max().item() < 2e-4 * r.abs().max().item()
    with torch.no_grad():
        o = DC.dc_unet_forward(P, cfg, T("x").double(), T("t"), T("context").double(), fs=None, default_fs=10)
        assert (o - T("out_default_fs").double()).abs().max().item() < 2e-5 * ref.abs().max().item()
        o = DC.dc_unet_forward(P, cfg, T("x").double(), T("t"), T("context_shared").double(), fs=T("fs"))
        assert (o - T("out_shared").double()).abs().max().item() < 2e-5 * ref.abs().max().item()


def test_dc_cross_attention_restatement_matches_reference_module():
    """CrossAttention(img_cross_attention=True) alone: output, both input gradients, every parameter gradient"""
    cfg, P = _dc_params()
    g = np.load(os.path.join(golden_io.GOLDEN, "dc_xattn.npz"))
    pre = str(g["prefix"])
    for v in P.values():
        v.requires_grad_(True)
    T = lambda k: torch.from_numpy(g[k]).double()
    x, ctx = T("in0").requires_grad_(True), T("in1").requires_grad_(True)
    y = DC.dc_cross_attention(x, P, pre, 1, ctx)
    assert (y - T("y")).abs().max().item() < 2e-5 * T("y").abs().max().item()
    (y * T("gy")).sum().backward()
    for got, k in ((x.grad, "gin0"), (ctx.grad, "gin1")):
        assert (got - T(k)).abs().max().item() < 1e-4 * T(k).abs().max().item(), k
    keys = [k for k in g.files if k.startswith("g.")]
    assert sorted(k[2:] for k in keys) == sorted(["to_q.weight", "to_k.weight", "to_v.weight", "to_out.0.weight", "to_out.0.bias",
                                                   "to_k_ip.weight", "to_v_ip.weight"])
    for k in keys:
        assert (P[pre + "." + k[2:]].grad - T(k)).abs().max().item() < 1e-4 * T(k).abs().max().item(), k


def test_dc_unet_parameter_names_and_order_equal_the_reference():
    """vt355.unet.UNetModel(img_cross_attention, fs_condition, in_channels 8): named_parameters() == the reference module's list stored
    in the golden, so its checkpoints load with strict=True"""
    from vt355.unet import UNetModel
    cfg = DC.dc_tiny_config()
    m = UNetModel(in_channels=8, out_channels=4, model_channels=cfg.model_channels, attention_resolutions=list(cfg.attention_resolutions),
                  num_res_blocks=cfg.num_res_blocks, channel_mult=list(cfg.channel_mult), dropout=0.1, num_head_channels=64,
                  transformer_depth=1, context_dim=cfg.context_dim, use_linear=True, use_checkpoint=True, temporal_conv=True,
                  temporal_attention=True, temporal_selfatt_only=True, use_relative_position=False, use_causal_attention=False,
                  temporal_length=cfg.temporal_length, addition_attention=True, img_cross_attention=True, default_fs=10, fs_condition=True)
    names = [str(n) for n in golden_io.load("dc_unet_tiny")["names"]]
    assert [n for n, _ in m.named_parameters()] == names
    P = DC.dc_init_params(cfg, seed=21, dtype=torch.bfloat16)
    m.load_state_dict(P, strict=True)
    assert torch.equal(dict(m.named_parameters())["middle_block.1.transformer_blocks.0.attn2.to_v_ip.weight"],
                       P["middle_block.1.transformer_blocks.0.attn2.to_v_ip.weight"])
    with pytest.raises(NotImplementedError):
        UNetModel(in_channels=8, out_channels=4, model_channels=64, attention_resolutions=[1], num_res_blocks=1, channel_mult=[1],
                  num_head_channels=64, context_dim=64, use_linear=True, use_relative_position=False, temporal_length=4,
                  img_cross_attention=True, img_cross_attention_scale_learnable=True)
    with pytest.raises(NotImplementedError):
        m.add_lora()


def _reference_yaml():
    """the recipe as the reference ships it: read from the reference tree where it is present (the build box), else the byte-identical
    settings-only copy under tests/golden/"""
    ref = "/root/reference/configs/002_dynamicrafter/dc_i2v_1024.yaml"
    local = os.path.join(golden_io.GOLDEN, "dc_i2v_1024.yaml")
    if os.path.exists(ref):
        assert open(ref, "rb").read() == open(local, "rb").read(), "tests/golden/dc_i2v_1024.yaml is no longer the reference's file"
    return local


def test_recipe_yaml_loads_unchanged():
    """configs/002_dynamicrafter/dc_i2v_1024.yaml, whole: model.target resolves to vt355.lvdm.LatentVisualDiffusionFlow, which builds the UNet,
    the zero-terminal-SNR scheduler and the Resampler from their nodes and records (does not build) the frozen VAE / OpenCLIP nodes"""
    from vt355.config import instantiate_from_config, load_yaml
    from vt355.lvdm import LatentVisualDiffusionFlow
    from vt355.resampler import Resampler
    from vt355.unet import UNetModel
    cfg = load_yaml(_reference_yaml())
    assert cfg["model"]["target"] == "videotuna.models.lvdm.ddpm3d.LatentVisualDiffusionFlow"
    with torch.device("meta"):
        flow = instantiate_from_config(cfg["model"])
    assert isinstance(flow, LatentVisualDiffusionFlow) and isinstance(flow.model, UNetModel) and isinstance(flow.image_proj_model, Resampler)
    m = flow.model
    assert m.config.img_cross_attention and m.config.fs_condition and m.config.default_fs == 10 and m.in_channels == 8 and m.config.dropout == 0.1
    n_ip = sum(1 for n in m.shapes if n.endswith("to_k_ip.weight"))
    assert n_ip == 16 and m.shapes["input_blocks.1.1.transformer_blocks.0.attn2.to_k_ip.weight"] == (320, 1024)
    r = flow.image_proj_model
    assert r.shapes["latents"] == (1, 256, 1024) and r.shapes["proj_in.weight"] == (1024, 1280) and r.config.depth == 4 and r.config.heads == 12
    assert flow.scheduler.rescale_betas_zero_snr and float(flow.scheduler.alphas_cumprod[-1]) == 0.0
    assert flow.parameterization == "v" and flow.use_scale and flow.scale_arr.shape == (1400,) and flow.uncond_prob == 0.05
    assert flow.rand_cond_frame and flow.fps_condition_type == "fps" and flow.image_proj_model_trainable
    fz = flow.frozen_stage_configs
    assert fz["first_stage_config"]["target"].endswith("AutoencoderKL") and fz["cond_stage_config"]["target"].endswith("FrozenOpenCLIPEmbedder")
    assert fz["img_cond_stage_config"]["target"].endswith("FrozenOpenCLIPImageEmbedderV2")


def test_three_way_condition_dropout_masks_equal_the_golden():
    """LatentVisualDiffusionFlow.condition_masks for a fixed random_num vector (thresholds at p, 2p, 3p hit exactly) vs the reference's
    expressions evaluated by tests/golden/make_golden_dc.py; and drop_conditions replaces exactly those samples"""
    from vt355.lvdm import LatentVisualDiffusionFlow
    g = np.load(os.path.join(golden_io.GOLDEN, "dc_masks.npz"))
    flow = LatentVisualDiffusionFlow.__new__(LatentVisualDiffusionFlow)
    torch.nn.Module.__init__(flow)
    flow.uncond_prob, flow.null_context, flow.null_image_tokens = float(g["uncond_prob"]), None, None
    r = torch.from_numpy(g["random_num"])
    drop_text, keep_image = flow.condition_masks(r)
    assert np.array_equal(drop_text.numpy(), g["prompt_mask"].astype(bool))
    assert np.array_equal(keep_image.numpy().astype(np.float32), g["input_mask"].astype(np.float32))
    assert drop_text.sum() == 6 and (~keep_image).sum() == 6 and (drop_text & ~keep_image).sum() == 3          # text only / both / image only
    B = r.shape[0]
    ctx, tok = torch.randn(B, 5, 8), torch.randn(B, 7, 4)
    nctx, ntok = torch.full((5, 8), 3.0), torch.full((7, 4), -2.0)
    c2, t2 = flow.drop_conditions(ctx, tok, r, nctx, ntok)
    for b in range(B):
        assert torch.equal(c2[b], nctx if drop_text[b] else ctx[b]) and torch.equal(t2[b], tok[b] if keep_image[b] else ntok)
    with pytest.raises(RuntimeError):
        flow.drop_conditions(ctx, tok, r, nctx, None)


def test_zero_terminal_snr_schedule():
    """rescale_betas_zero_snr: True equals the reference's table (float64, rtol 1e-12), ends at exactly 0; False is what it always was"""
    from vt355.lvdm import LDDPM
    g = np.load(os.path.join(golden_io.GOLDEN, "dc_schedule.npz"))
    on = LDDPM(timesteps=1000, linear_start=0.00085, linear_end=0.012, rescale_betas_zero_snr=True)
    assert on.alphas_cumprod.dtype == torch.float64
    assert np.allclose(on.alphas_cumprod.numpy(), g["alphas_cumprod_zero_snr"], rtol=1e-12, atol=0)
    assert float(on.alphas_cumprod[-1]) == 0.0
    off = LDDPM(timesteps=1000, linear_start=0.00085, linear_end=0.012, rescale_betas_zero_snr=False)
    dflt = LDDPM(timesteps=1000, linear_start=0.00085, linear_end=0.012)
    plain = np.cumprod(1.0 - np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2, axis=0)
    assert np.array_equal(off.alphas_cumprod.numpy(), plain) and np.array_equal(dflt.alphas_cumprod.numpy(), plain)
    assert np.allclose(plain, np.cumprod(1.0 - g["betas"], axis=0), rtol=1e-12, atol=0)          # the reference's own unrescaled table
    assert not np.allclose(on.alphas_cumprod.numpy(), plain, rtol=1e-3)


def test_resampler_restatement_matches_reference_module():
    """tests/dc_oracle.rs_forward vs ip_resampler.Resampler (tiny, frame-wise queries): output and every parameter gradient"""
    g = golden_io.load("dc_resampler")
    P = {k: v.double().requires_grad_(True) for k, v in DC.rs_init_params(DC.RS_TINY, seed=31).items()}
    assert [str(n) for n in g["names"]] == list(P)
    T = lambda k: torch.from_numpy(g[k]).double()
    y = DC.rs_forward(P, DC.RS_TINY, T("x"))
    assert (y - T("y")).abs().max().item() < 2e-5 * T("y").abs().max().item()
    (y * T("gy")).sum().backward()
    for n in P:
        r = T("g." + n)
        assert (P[n].grad - r).abs().max().item() < 2e-4 * r.abs().max().item() + 1e-9, n


def test_resampler_parameter_names_and_order_equal_the_reference():
    from vt355.resampler import Resampler
    m = Resampler(**DC.RS_TINY)
    assert [n for n, _ in m.named_parameters()] == [str(n) for n in golden_io.load("dc_resampler")["names"]]
    m.load_state_dict(DC.rs_init_params(DC.RS_TINY, seed=31), strict=True)
    with pytest.raises(NotImplementedError):
        Resampler(dim_head=32)
