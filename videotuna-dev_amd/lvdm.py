"""VideoCrafter2 training workflow on the vt355 UNet: the part of ``LVDMFlow`` / ``VideocrafterFlow`` that runs inside
``training_step`` (videotuna/models/lvdm/ddpm3d.py:732-741, 787-868; videotuna/flow/videocrafter.py:418-487) --
``t ~ U{0..T-1}`` -> dynamic rescaling ``x * scale_arr[t]`` (use_scale) -> ``q_sample`` -> UNet -> eps / v / x0 target ->
``mean_b mean_rest (pred - target)^2`` (logvar == 0, l_simple_weight 1, original_elbo_weight 0).

Same constructor keys as the reference classes for what this path needs (``unet_config`` / ``denoiser_config``,
``scheduler_config`` / ``diffusion_scheduler_config``, ``use_scale``, ``scale_a``, ``scale_b``, ``parameterization``, ...), so that
``configs/001_videocrafter2/vc2_t2v_320x512.yaml`` (flow style) and ``vc2_t2v_lora.yaml`` (model style) instantiate through
``vt355.config.instantiate_from_config``; everything else in those nodes (VAE, CLIP embedder, EMA, logging keys) is accepted and
ignored: the frozen first / cond stages are outside this path, batches carry pre-encoded ``{"latents" [B,4,T,H,W], "context"
[B,77,1024][, "fps"]}``.  Full fine-tuning (the flow-style recipe) or, with ``lora_args`` (vc2_t2v_lora.yaml:7-12), rank-r adapters on to_q / to_k / to_v
of every CrossAttention with the base weights frozen (ddpm3d.py:100-117, 434-445): ``inject_lora()`` wraps the denoiser the way
``peft.get_peft_model(DiffusionWrapper(unet))`` names things -- ``model.base_model.model.diffusion_model.<path>.to_q.lora_A.default.weight`` --
so LoRA-only checkpoints (videotuna/utils/callbacks.py:28-53) and ``load_lora_from_ckpt`` (ddpm3d.py:406-432) interchange.

Classifier-free-guidance dropout of the condition (``uncond_prob``, default 0.2; ddpm3d.py:460-461, 710-722): ``empty_seq`` replaces a sample's
caption by "" BEFORE the frozen text encoder, so on pre-encoded batches its context rows are replaced by the embedding of the empty prompt,
which the batch (``"null_context"`` [77, 1024] or [B, 77, 1024]) or the constructor (``null_context=``) must supply; ``zero_embed`` zeroes them.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .config import instantiate_from_config
from .optim import FusedAdamW


def zero_terminal_snr_betas(betas: np.ndarray) -> np.ndarray:
    """Algorithm 1 of "Common Diffusion Noise Schedules and Sample Steps are Flawed" (arXiv 2305.08891), as the reference applies it for
    ``rescale_betas_zero_snr: True`` (schedulers/ddpm.py:83, utils/diffusion_utils.py:141): sqrt(abar) is shifted so that its last value is
    zero and rescaled so that its first value is kept; float64 throughout.  The last alphas_cumprod is then exactly 0."""
    root = np.sqrt(np.cumprod(1.0 - np.asarray(betas, dtype=np.float64), axis=0))
    first, last = root[0].copy(), root[-1].copy()
    root = (root - last) * (first / (first - last))
    abar = root ** 2
    alphas = np.concatenate([abar[0:1], abar[1:] / abar[:-1]])
    return 1.0 - alphas


class LDDPM:
    """schedule tables of videotuna/schedulers/ddpm.py:64-153 (beta_schedule "linear": linspace(sqrt(s), sqrt(e))^2, float64) and
    q_sample / get_v (:216-228)"""

    def __init__(self, timesteps: int = 1000, beta_schedule: str = "linear", linear_start: float = 1e-4, linear_end: float = 2e-2,
                 parameterization: str = "eps", rescale_betas_zero_snr: bool = False, **unused):
        if beta_schedule != "linear":
            raise NotImplementedError("only the 'linear' beta schedule of the VideoCrafter2 recipes is built")
        self.num_timesteps = int(timesteps)
        self.parameterization = parameterization
        self.rescale_betas_zero_snr = bool(rescale_betas_zero_snr)
        betas = np.linspace(linear_start ** 0.5, linear_end ** 0.5, timesteps, dtype=np.float64) ** 2
        if self.rescale_betas_zero_snr:
            betas = zero_terminal_snr_betas(betas)
        self.alphas_cumprod = torch.from_numpy(np.cumprod(1.0 - betas, axis=0))
        self.logvar = torch.zeros(timesteps)
        self.learn_logvar = False
        self._dev = {}

    def coefficients(self, t: torch.Tensor):
        """(sqrt(abar_t), sqrt(1 - abar_t)) as fp32 device vectors [B]"""
        dev = t.device
        if dev not in self._dev:
            a = self.alphas_cumprod
            self._dev[dev] = torch.stack([a.sqrt(), (1 - a).sqrt()]).to(torch.float32).to(dev)
        sel = self._dev[dev][:, t]
        return sel[0].contiguous(), sel[1].contiguous()


LDMScheduler = LDDPM          # videotuna.schedulers.diffusion_schedulers.LDMScheduler: the same tables as a LightningModule


class _EpsLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        loss = torch.empty(1, dtype=torch.float32, device=pred.device)
        dp = torch.empty_like(pred)
        ops.mse_loss(pred.contiguous(), target, loss, dp)
        ctx.save_for_backward(dp)
        return loss.view(())

    @staticmethod
    def backward(ctx, gout):
        (dp,) = ctx.saved_tensors
        return dp * gout.to(dp.dtype), None


class _Holder(nn.Module):
    pass


class _PeftUNet(nn.Module):
    """what ``peft.get_peft_model(DiffusionWrapper(unet), lora_config)`` looks like from outside (ddpm3d.py:99, 434-440): the UNet sits at
    ``base_model.model.diffusion_model``, so parameter names read ``base_model.model.diffusion_model.<path>.to_q.lora_A.default.weight``
    (base weights keep ``<path>.to_q.weight``; peft's ``base_layer`` level is not reproduced -- only "lora" keys are ever saved or loaded)"""

    def __init__(self, unet):
        super().__init__()
        self.base_model = _Holder()
        self.base_model.model = _Holder()
        self.base_model.model.diffusion_model = unet

    @property
    def unet(self):
        return self.base_model.model.diffusion_model

    def forward(self, *a, **k):
        return self.unet(*a, **k)

    @property
    def device(self):
        return self.unet.device

    def print_trainable_parameters(self):
        self.unet.print_trainable_parameters()

    def lora_weights_changed(self):
        self.unet.lora.weights_changed()


class LVDMFlow(nn.Module):
    def __init__(self, unet_config=None, denoiser_config=None, scheduler_config=None, diffusion_scheduler_config=None,
                 use_scale: bool = False, scale_a: float = 1.0, scale_b: float = 0.3, mid_step: int = 400, fix_scale_bug: bool = False,
                 parameterization: Optional[str] = None, base_learning_rate: float = 6e-6, lora_args=None, logdir=None,
                 l_simple_weight: float = 1.0, original_elbo_weight: float = 0.0, uncond_prob: float = 0.2, uncond_type: str = "empty_seq",
                 null_context=None, **ignored):
        super().__init__()
        if original_elbo_weight != 0.0 or l_simple_weight != 1.0:
            raise NotImplementedError("only l_simple_weight 1 / original_elbo_weight 0 (the shipped recipes) are built")
        if uncond_type not in ("empty_seq", "zero_embed"):
            raise ValueError(f"uncond_type {uncond_type!r}: 'empty_seq' or 'zero_embed' (ddpm3d.py:710-722)")
        node = denoiser_config if denoiser_config is not None else unet_config
        self.model = instantiate_from_config(node)
        self.model.bfloat16()
        # peft lora config, argument names as the reference's (ddpm3d.py:100-117); injected by inject_lora() as scripts/train.py:168-169 does
        self.lora_args = dict(lora_args) if lora_args else {}
        if self.lora_args:
            self.lora_ckpt_path = self.lora_args.get("lora_ckpt", None)
            self.lora_rank = int(self.lora_args.get("lora_rank", 4))
            self.lora_alpha = float(self.lora_args.get("lora_alpha", 1))
            self.lora_dropout = float(self.lora_args.get("lora_dropout", 0.0))
            self.target_modules = list(self.lora_args.get("target_modules", ["to_k", "to_v", "to_q"]))
            if self.lora_dropout != 0.0:
                raise NotImplementedError("lora_dropout > 0 is not built (the shipped recipe uses 0.0)")
        self.uncond_prob, self.uncond_type = float(uncond_prob), uncond_type
        self.null_context = None if null_context is None else torch.as_tensor(null_context)
        sch = scheduler_config if scheduler_config is not None else diffusion_scheduler_config
        self.scheduler = instantiate_from_config(sch) if sch is not None else LDDPM(linear_start=0.00085, linear_end=0.012)
        self.diffusion_scheduler = self.scheduler
        self.parameterization = parameterization or getattr(self.scheduler, "parameterization", "eps")
        self.num_timesteps = self.scheduler.num_timesteps
        self.use_scale = use_scale
        if use_scale:      # ddpm3d.py:500-514 (the reference's default keeps the 1400-long table: fix_scale_bug False)
            step = self.num_timesteps - mid_step if fix_scale_bug else self.num_timesteps
            arr = np.concatenate((np.linspace(scale_a, scale_b, mid_step), np.full(step, scale_b)))
            self.register_buffer("scale_arr", torch.tensor(arr, dtype=torch.float32))
        self.learning_rate = base_learning_rate
        self.logdir = logdir
        self.global_step = 0

    @property
    def device(self):
        return self.model.device

    @property
    def unet(self):
        return self.model.unet if isinstance(self.model, _PeftUNet) else self.model

    def inject_lora(self):
        """ddpm3d.py:434-445: adapters into the denoiser (not the condition model), every other weight frozen, optional resume"""
        if not self.lora_args:
            raise RuntimeError("inject_lora() without lora_args in the model config")
        if isinstance(self.model, _PeftUNet):
            return
        unet = self.model
        unet.add_lora(self.lora_rank, self.lora_alpha, self.target_modules)
        self.model = _PeftUNet(unet)
        self.model.print_trainable_parameters()
        if self.lora_ckpt_path is not None:
            self.load_lora_from_ckpt(self.model, self.lora_ckpt_path)

    def load_lora_from_ckpt(self, model, path):
        from .checkpoint import load_lora_from_ckpt
        return load_lora_from_ckpt(model, path)

    def on_save_checkpoint(self, checkpoint):
        """LoraModelCheckpoint's rule (videotuna/utils/callbacks.py:44-46): with adapters present only "lora" keys are written"""
        sd = {k: v for k, v in checkpoint["state_dict"].items() if "lora" in k}
        if sd:
            checkpoint["state_dict"] = sd
        return checkpoint

    def configure_optimizers(self, gradient_clip_val=None, gradient_clip_algorithm="norm"):
        """gradient_clip_val / gradient_clip_algorithm: Lightning's trainer options (config.trainer_options reads them from a recipe)"""
        if isinstance(self.model, _PeftUNet):
            ts = self.unet.enable_lora_training()
        else:
            ts = self.model.enable_training()
        return FusedAdamW(ts.params, lr=self.learning_rate, fullft_state=ts, gradient_clip_val=gradient_clip_val, gradient_clip_algorithm=gradient_clip_algorithm)

    def p_losses(self, x_start, context, t, noise, fps=16):
        """x_start fp32 [B,C,T,H,W] (already multiplied by scale_arr[t] when use_scale -- done in forward(), ddpm3d.py:740-741)"""
        sa, sb = self.scheduler.coefficients(t)
        x_noisy = torch.empty(x_start.shape, dtype=torch.bfloat16, device=x_start.device)
        ops.q_sample(x_start, noise, sa, sb, None, x_noisy)
        out = self.model(x_noisy, t, context=context, fps=fps)
        if self.parameterization == "eps":
            target = noise
        elif self.parameterization == "x0":
            target = x_start
        else:                       # "v": sqrt(abar) eps - sqrt(1-abar) x0   (schedulers/ddpm.py:224-228)
            target = sa.view(-1, 1, 1, 1, 1) * noise - sb.view(-1, 1, 1, 1, 1) * x_start
        return _EpsLoss.apply(out, target.contiguous())

    def loss_from(self, z, context, t, noise, fps=16):
        """deterministic core of training_step (fixed t / noise): what the parity tests call"""
        z = z.to(torch.float32)
        if self.use_scale:
            z = z * self.scale_arr[t].view(-1, 1, 1, 1, 1)
        return self.p_losses(z.contiguous(), context, t, noise.to(torch.float32).contiguous(), fps)

    def training_step(self, batch, batch_idx=0):
        if "latents" not in batch:
            raise RuntimeError("the VideoCrafter2 path takes pre-encoded batches {'latents','context'[,'fps']}: the frozen 2-D VAE and "
                               "the OpenCLIP embedder of the reference recipe are outside this engine's hot path (SURVEY 8(f))")
        z = batch["latents"]
        B = z.shape[0]
        context = self.random_uncond(batch["context"], batch.get("null_context"))
        t = torch.randint(0, self.num_timesteps, (B,), device=z.device).long()
        noise = torch.randn(z.shape, dtype=torch.float32, device=z.device)
        return self.loss_from(z, context, t, noise, batch.get("fps", 16))

    def random_uncond(self, context, null_context=None, drop=None):
        """shared_step(random_uncond = uncond_prob > 0) of the reference (ddpm3d.py:534-535, 710-722): per sample, with probability uncond_prob,
        the condition becomes the unconditional one -- the encoding of "" (empty_seq; pre-encoded here) or zeros (zero_embed).  ``drop``
        (bool [B]) fixes the draw (tests); otherwise one python ``random.random()`` per sample, as the reference."""
        if self.uncond_prob <= 0.0 or not self.training:
            return context
        import random
        B = context.shape[0]
        if drop is None:
            drop = torch.tensor([random.random() < self.uncond_prob for _ in range(B)])
        drop = torch.as_tensor(drop, dtype=torch.bool)
        if not bool(drop.any()):
            return context
        if self.uncond_type == "zero_embed":
            null = torch.zeros_like(context[0])
        else:
            null = null_context if null_context is not None else self.null_context
            if null is None:
                raise RuntimeError("uncond_prob > 0 with uncond_type 'empty_seq' needs the embedding of the empty prompt: put it in the batch "
                                   "('null_context' [77, C]) or give the workflow null_context=; or set uncond_prob: 0.0 (no classifier-free-"
                                   "guidance dropout -- NOT what the reference trains, ddpm3d.py:460)")
            null = null.to(device=context.device, dtype=context.dtype)
        if null.dim() == context.dim():
            null_b = null
        else:
            null_b = null.unsqueeze(0).expand_as(context)
        return torch.where(drop.to(context.device).view(B, *([1] * (context.dim() - 1))), null_b, context)


VideocrafterFlow = LVDMFlow


class _JointOptimizer:
    """the fused AdamW of every trained module of a flow (the UNet, the Resampler) behind one optimizer interface: each module keeps its own
    flat master / gradient buffer, so a step is one fused launch per module.

    Gradient clipping by norm is over ALL parameters of the step, as Lightning's: every member's norm pass writes into one array of
    partial sums, one finalise leaves the joint norm and its coefficient in device memory, and every member's AdamW launch reads that
    same coefficient.  The members must have been built with the same clip settings."""

    def __init__(self, optimizers):
        self.optimizers = list(optimizers)
        self.param_groups = [g for o in self.optimizers for g in o.param_groups]
        if len({(o.gradient_clip_val or None, o.gradient_clip_algorithm) for o in self.optimizers}) != 1:
            raise ValueError("the optimizers of one step clip together: give every member the same gradient_clip_val / gradient_clip_algorithm, got "
                             + ", ".join(f"({o.gradient_clip_val!r}, {o.gradient_clip_algorithm!r})" for o in self.optimizers))

    @property
    def gradient_clip_val(self):
        return self.optimizers[0].gradient_clip_val

    @property
    def gradient_clip_algorithm(self):
        return self.optimizers[0].gradient_clip_algorithm

    @property
    def grad_norm(self):
        """0-dim device tensor: the joint pre-clip gradient norm of the last step (None unless 'norm' clipping is on)"""
        return self.optimizers[0].grad_norm

    def zero_grad(self, set_to_none: bool = False):
        for o in self.optimizers:
            o.zero_grad(set_to_none)

    def step(self, closure=None, grad_scale: float = 1.0):
        first = self.optimizers[0]
        if first._clip_mode() != "norm":
            for o in self.optimizers:
                o.step(closure, grad_scale)
            return
        if closure is not None:
            closure()
        self.check_errors()
        partials, record = first._clip_buffers(sum(len(o._grad_buffers()) for o in self.optimizers))
        slot = 0
        for o in self.optimizers:
            slot = o._norm_pass(partials, slot)
        ops.clip_finalize(partials, slot, grad_scale, float(first.gradient_clip_val), record)
        for o in self.optimizers:
            o._clip_record = record            # every member's grad_norm is the joint one
            o.step(grad_scale=grad_scale, clip_coef=record[1:2])

    def check_errors(self, wait: bool = True):
        for o in self.optimizers:
            o.check_errors(wait)


class LatentVisualDiffusionFlow(LVDMFlow):
    """DynamiCrafter's image-to-video flow (videotuna/models/lvdm/ddpm3d.py:1311-1480 get_batch_input, :787-848 p_losses) on pre-encoded
    batches ``{'latents' [B,4,T,H,W], 'context' [B,77,C], 'image_tokens' [B,257,1280], 'fps' | 'frame_stride' [B]}`` (optionally
    ``'cond_frame_index'``, ``'null_context'``, ``'null_image_tokens'``).  The frozen 2-D VAE and the OpenCLIP text / image towers stay outside
    (their config nodes are recorded in ``frozen_stage_configs``, not instantiated); the image-context projector (``image_proj_stage_config``:
    vt355.resampler.Resampler) is part of the flow and trains with the UNet when ``image_proj_model_trainable``.

    The reference zeroes the conditioning IMAGE of a sample whose image condition is dropped and encodes it; with pre-encoded tokens the
    caller supplies that encoding once as ``null_image_tokens`` [257, 1280] (the image tower's output for an all-zero image)."""

    def __init__(self, img_cond_stage_config=None, finegrained=False, image_proj_stage_config=None, freeze_embedder=True,
                 image_proj_model_trainable=True, rand_cond_frame: bool = False, fps_condition_type: str = "fs", interp_mode: bool = False,
                 conditioning_key: str = "hybrid", null_image_tokens=None, first_stage_config=None, cond_stage_config=None, **kwargs):
        if kwargs.get("lora_args"):
            raise NotImplementedError("LoRA on the DynamiCrafter flow: the reference ships no such recipe")
        super().__init__(**kwargs)
        if image_proj_stage_config is None or finegrained:
            raise NotImplementedError("only the Resampler projector of the DynamiCrafter recipe (image_proj_stage_config) is built")
        if interp_mode:
            raise NotImplementedError("interp_mode is not built")
        if conditioning_key != "hybrid":
            raise NotImplementedError("conditioning_key 'hybrid' (concat of the conditioning frame's latent + cross-attention) is the recipe's")
        if fps_condition_type not in ("fs", "fps"):
            raise ValueError(f"fps_condition_type {fps_condition_type!r}: 'fs' (batch['frame_stride']) or 'fps' (batch['fps'])")
        self.frozen_stage_configs = dict(img_cond_stage_config=img_cond_stage_config, first_stage_config=first_stage_config,
                                         cond_stage_config=cond_stage_config, freeze_embedder=freeze_embedder)
        self.image_proj_model = instantiate_from_config(image_proj_stage_config)
        self.image_proj_model.bfloat16()
        self.image_proj_model_trainable = bool(image_proj_model_trainable)
        self.rand_cond_frame, self.fps_condition_type, self.conditioning_key = bool(rand_cond_frame), fps_condition_type, conditioning_key
        self.null_image_tokens = None if null_image_tokens is None else torch.as_tensor(null_image_tokens)

    def configure_optimizers(self, gradient_clip_val=None, gradient_clip_algorithm="norm"):
        """gradient_clip_val / gradient_clip_algorithm: Lightning's trainer options; the recipe (dc_i2v_1024.yaml) clips the joint
        UNet + Resampler gradient norm at 0.5 (config.trainer_options reads them)"""
        clip = dict(gradient_clip_val=gradient_clip_val, gradient_clip_algorithm=gradient_clip_algorithm)
        ts = self.model.enable_training()
        opts = [FusedAdamW(ts.params, lr=self.learning_rate, fullft_state=ts, **clip)]
        if self.image_proj_model_trainable:
            rs = self.image_proj_model.enable_training()
            opts.append(FusedAdamW(rs.params, lr=self.learning_rate, fullft_state=rs, **clip))
        return _JointOptimizer(opts)

    def condition_masks(self, random_num: torch.Tensor):
        """ddpm3d.py:1391-1397: text dropped where r < 2p, image dropped where p <= r < 3p (p = uncond_prob): 5 % text only, 5 % both, 5 % image
        only at the recipe's p = 0.05.  Returns (drop_text bool [B], keep_image bool [B])"""
        p = self.uncond_prob
        drop_text = random_num < 2 * p
        keep_image = ~((random_num >= p) & (random_num < 3 * p))
        return drop_text, keep_image

    def drop_conditions(self, context, image_tokens, random_num, null_context=None, null_image_tokens=None):
        drop_text, keep_image = self.condition_masks(random_num)
        B = context.shape[0]
        if bool(drop_text.any()):
            null = null_context if null_context is not None else self.null_context
            if null is None:
                raise RuntimeError("dropping the text condition needs the embedding of the empty prompt: batch['null_context'] [77, C] or null_context=")
            null = null.to(device=context.device, dtype=context.dtype)
            context = torch.where(drop_text.to(context.device).view(B, 1, 1), null.expand_as(context) if null.dim() == 3 else null.unsqueeze(0).expand_as(context), context)
        if not bool(keep_image.all()):
            null = null_image_tokens if null_image_tokens is not None else self.null_image_tokens
            if null is None:
                raise RuntimeError("dropping the image condition needs the image tower's tokens of an all-zero image: batch['null_image_tokens'] "
                                   "[257, 1280] or null_image_tokens=")
            null = null.to(device=image_tokens.device, dtype=image_tokens.dtype)
            image_tokens = torch.where(keep_image.to(image_tokens.device).view(B, 1, 1), image_tokens,
                                       null.expand_as(image_tokens) if null.dim() == 3 else null.unsqueeze(0).expand_as(image_tokens))
        return context, image_tokens

    def loss_from(self, z, context, image_tokens, t, noise, fs=None, cond_frame_index: int = 0):
        """deterministic core of training_step (fixed t / noise / conditioning frame): Resampler -> context = [text | image tokens per frame],
        hybrid input = [q_sample(z * scale) | latent of the conditioning frame repeated over time], UNet, v / eps / x0 MSE"""
        z = z.to(torch.float32)
        B, C, T = z.shape[:3]
        img_ctx = self.image_proj_model(image_tokens.to(torch.bfloat16).contiguous())                    # [B, T*16, ctx]
        ctx = torch.cat([context.to(torch.bfloat16), img_ctx], dim=1)
        cond = z[:, :, cond_frame_index:cond_frame_index + 1].expand(B, C, T, *z.shape[3:])             # c_concat: from z BEFORE use_scale
        x_start = (z * self.scale_arr[t].view(-1, 1, 1, 1, 1) if self.use_scale else z).contiguous()
        noise = noise.to(torch.float32).contiguous()
        sa, sb = self.scheduler.coefficients(t)
        x_noisy = torch.empty(x_start.shape, dtype=torch.bfloat16, device=z.device)
        ops.q_sample(x_start, noise, sa, sb, None, x_noisy)
        x_in = torch.cat([x_noisy, cond.to(torch.bfloat16)], dim=1).contiguous()
        out = self.model(x_in, t, context=ctx, fs=None if fs is None else torch.as_tensor(fs, device=z.device).long())
        if self.parameterization == "eps":
            target = noise
        elif self.parameterization == "x0":
            target = x_start
        else:
            target = sa.view(-1, 1, 1, 1, 1) * noise - sb.view(-1, 1, 1, 1, 1) * x_start
        return _EpsLoss.apply(out, target.contiguous())

    def training_step(self, batch, batch_idx=0):
        for k in ("latents", "context", "image_tokens"):
            if k not in batch:
                raise RuntimeError("the DynamiCrafter path takes pre-encoded batches {'latents', 'context', 'image_tokens', 'fps' | 'frame_stride'}: "
                                   "the frozen 2-D VAE and the OpenCLIP text / image towers are outside this engine's hot path")
        z = batch["latents"]
        B, T = z.shape[0], z.shape[2]
        context, tokens = batch["context"], batch["image_tokens"]
        if self.training and self.uncond_prob > 0.0:                      # shared_step(random_uncond=True)
            context, tokens = self.drop_conditions(context, tokens, torch.rand(B, device=z.device), batch.get("null_context"),
                                                   batch.get("null_image_tokens"))
        idx = batch.get("cond_frame_index")
        if idx is None:
            import random
            idx = random.randint(0, T - 1) if self.rand_cond_frame else 0
        fs = batch["frame_stride"] if self.fps_condition_type == "fs" else batch["fps"]
        t = torch.randint(0, self.num_timesteps, (B,), device=z.device).long()
        noise = torch.randn(z.shape, dtype=torch.float32, device=z.device)
        return self.loss_from(z, context, tokens, t, noise, fs, int(idx))
