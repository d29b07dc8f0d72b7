"""Shared by tests/test_grad_clip_cpu.py and tests/test_grad_clip_gpu.py (not a test module)."""
import math

import torch

from parity import close  # noqa: F401  (the comparison of the gradient-clip tests: NaN and Inf are out of tolerance)

TREE_LEVELS = 10      # fp32 tree levels of vt_grad_sqnorm before the double stage: 4 lanes (2) + 64-wide wave (6) + 4 waves (2)
THREADS = 256


def sqnorm_rel_bound(n: int, blocks: int) -> float:
    """Relative error bound of the fp32 stage of the squared norm of n values (include/vt355.h states the scheme).  All terms are
    non-negative, so every rounding moves the running sum by at most 2^-24 of itself and the errors add: each g*g is rounded once (1),
    a thread adds at most m = ceil(ceil(n / 4) / (blocks * 256)) + 1 terms into one accumulator (the + 1 is a head or tail element),
    and t = 10 tree levels follow; the double stage adds nothing at this scale.  (m + t + 1) * 2^-24 for the sum, half of it for the norm."""
    m = math.ceil(math.ceil(n / 4) / (blocks * THREADS)) + 1
    return (m + TREE_LEVELS + 1) * 2.0 ** -24


def tiny_dc_flow():
    """the tiny DynamiCrafter flow of tests/test_dc_gpu.py (seeded weights), on the CPU; move it with .to(dev)"""
    import dc_oracle as DC
    from vt355.lvdm import LatentVisualDiffusionFlow
    cfg = DC.dc_tiny_config()
    unet = dict(target="vt355.unet.UNetModel", params=dict(
        in_channels=8, out_channels=4, model_channels=cfg.model_channels, attention_resolutions=list(cfg.attention_resolutions),
        num_res_blocks=cfg.num_res_blocks, channel_mult=list(cfg.channel_mult), dropout=0.1, num_head_channels=64, transformer_depth=1,
        context_dim=cfg.context_dim, use_linear=True, use_checkpoint=True, temporal_conv=True, temporal_attention=True,
        temporal_selfatt_only=True, use_relative_position=False, use_causal_attention=False, temporal_length=cfg.temporal_length,
        addition_attention=True, img_cross_attention=True, default_fs=10, fs_condition=True))
    flow = LatentVisualDiffusionFlow(
        unet_config=unet, image_proj_stage_config=dict(target="vt355.resampler.Resampler", params=dict(DC.RS_FLOW)),
        diffusion_scheduler_config=dict(target="vt355.lvdm.LDDPM", params=dict(timesteps=1000, linear_start=0.00085, linear_end=0.012,
                                                                              rescale_betas_zero_snr=True)),
        parameterization="v", use_scale=True, scale_b=0.3, uncond_prob=0.05, uncond_type="empty_seq", rand_cond_frame=True,
        fps_condition_type="fps", image_proj_model_trainable=True, base_learning_rate=1e-3)
    flow.model.load_state_dict(DC.dc_init_params(cfg, seed=21))
    flow.image_proj_model.load_state_dict(DC.rs_init_params(DC.RS_FLOW, seed=33))
    return cfg, flow
