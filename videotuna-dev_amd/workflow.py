"""``CogVideoXWorkFlow`` -- the training workflow of videotuna/models/cogvideo_hf/cogvideo_pl.py:90-149, 774-887 on the
vt355 engine: same constructor keys (so configs/004_cogvideox/*.yaml load unchanged through
``vt355.config.instantiate_from_config``), same ``training_step(batch, batch_idx) -> loss``,
``configure_optimizers()``, ``inject_adapter()``, ``on_save_checkpoint()`` (LoRA-only filter), ``lora_args``; and the sampling side
(cogvideo_pl.py:476-772, 890-899): ``sample(...)`` and, when the VAE directory holds a decoder, ``log_images(batch)``.

Scope: the frozen VAE and T5 encoders are NOT part of this hot path.  A batch is either
  * pre-encoded: {"latents": [B,C,F,H,W] (VAE sample * scaling_factor), "prompt_embeds": [B,226,4096]}  or
  * the reference schema {"video", "caption"} together with user-supplied ``first_stage`` / ``cond_stage`` callables.
"""
from __future__ import annotations

import math
import os
from typing import Any, Dict, Optional

import torch
import torch.nn as nn

from . import ops
from .config import instantiate_from_config
from .lora import LoraConfig, get_peft_model
from .optim import FusedAdamW
from .rope import prepare_rotary_positional_embeddings


class _LossFn(torch.autograd.Function):
    """loss = mean_b mean_i [ w_b (sqrt(abar) x_t - sqrt(1-abar) v - x0)^2 ]   (cogvideo_pl.py:872-886)."""

    @staticmethod
    def forward(ctx, vpred, noisy, x0, sa, sb, w):
        loss = torch.empty(1, dtype=torch.float32, device=vpred.device)
        part = torch.empty(512, dtype=torch.float32, device=vpred.device)
        ops.diffusion_loss(vpred, noisy, x0, sa, sb, w, loss, part, None)
        ctx.save_for_backward(vpred, noisy, x0, sa, sb, w)
        return loss.view(())

    @staticmethod
    def backward(ctx, gout):
        vpred, noisy, x0, sa, sb, w = ctx.saved_tensors
        dv = torch.empty_like(vpred)
        ops.diffusion_loss_bwd(vpred, noisy, x0, sa, sb, w, gout.reshape(1).to(torch.float32).contiguous(), dv)
        return dv, None, None, None, None, None


class CogVideoXWorkFlow(nn.Module):
    def __init__(self, first_stage_config=None, cond_stage_config=None, denoiser_config=None, scheduler_config=None,
                 learning_rate: float = 6e-6, adapter_config=None, logdir=None, first_stage=None, cond_stage=None,
                 cache_encodings: bool = False):
        super().__init__()
        self.logdir = logdir
        # opt-in per-sample cache of the frozen encoders' outputs (vt355.prefetch.EncodingCache): prompt embeddings by caption, latent
        # moments by the batch's "index" entry; steady-state epochs then run at the pre-encoded rate
        self.encoding_cache = None
        if cache_encodings:
            from .prefetch import EncodingCache
            self.encoding_cache = EncodingCache()
        self.learning_rate = learning_rate
        # frozen encoders: explicit callables win; else the config nodes are honoured when their checkpoints exist LOCALLY
        # (cogvideo_pl.py:104-121 builds them unconditionally; offline a model name such as "DeepFloyd/t5-v1_1-xxl" cannot
        # be fetched -> the stage stays None and batches must come pre-encoded, see get_batch_input)
        self.first_stage, self.cond_stage = first_stage, cond_stage
        self._first_stage_config = first_stage_config        # the decoder is built from it lazily (decode_latents / decode_first_stage)
        if first_stage is None and first_stage_config is not None:
            vae = self._optional_stage(first_stage_config)
            if vae is not None:
                self.vae = vae
                self.first_stage = vae.latents
        if cond_stage is None and cond_stage_config is not None:
            self.cond_stage_model = self._optional_stage(cond_stage_config)
            if self.cond_stage_model is not None:
                self.cond_stage = self.cond_stage_model
        self.vae_scale_factor_spatial, self.vae_scale_factor_temporal = 8, 4
        self.model = instantiate_from_config(denoiser_config)
        params = denoiser_config.get("params", {}) if isinstance(denoiser_config, dict) else {}
        # reference: load_dtype fp16 -> .half() (cogvideo_pl.py:125-132).  BASELINE fixes bf16 for this engine;
        # fp16 requests are served in bf16 (documented deviation).
        self.model.bfloat16()
        self.scheduler = instantiate_from_config(scheduler_config)
        self.lora_args = []
        if adapter_config is not None:
            self.inject_adapter(adapter_config)
        self.model.enable_gradient_checkpointing()
        self.global_step = 0
        self._rope_cache: Dict[tuple, Any] = {}

    @staticmethod
    def _optional_stage(node):
        """instantiate a frozen-encoder node, or None when it points at weights that are not on this machine"""
        params = (node.get("params") or {}) if isinstance(node, dict) else {}
        path = params.get("pretrained_model_name_or_path") or params.get("version")
        import os
        if path is None or not os.path.isdir(os.path.join(path, params.get("subfolder") or "")):
            return None
        try:
            return instantiate_from_config(node)
        except (KeyError, RuntimeError, ValueError, OSError) as e:
            # e.g. the reference's own HF download on disk: its VAE file carries diffusers' key names (encoder.down_blocks.N.resnets.M...),
            # which this encoder does not map (unverifiable offline).  The stage is optional: pre-encoded batches train without
            # it, and get_batch_input fails only when a raw {'video', 'caption'} batch really needs it.
            import warnings
            warnings.warn(f"frozen encoder {node.get('target') if isinstance(node, dict) else node} at {path} could not be loaded "
                          f"({type(e).__name__}: {str(e)[:200]}); the stage stays unset and batches must come pre-encoded")
            return None

    @property
    def dtype(self):
        return torch.bfloat16

    @property
    def device(self):
        return next(self.model.parameters()).device

    # ---- latents back to video (cogvideo_pl.py:162-172, 410-418) ----
    def _decoder_checkpoint(self):
        """the local file (or directory) ``first_stage_config`` names, or None"""
        node = getattr(self, "_first_stage_config", None)
        params = dict((node.get("params") or {}) if isinstance(node, dict) else {})
        root = params.get("pretrained_model_name_or_path") or params.get("path")
        path = os.path.join(root, params.get("subfolder") or "") if root else None
        return path if path is not None and os.path.exists(path) else None

    def _decodable(self) -> bool:
        """does ``first_stage_config`` name a local checkpoint with the decoder's weights?  Reads the file's key list only: the decoder
        itself is still built on the first decode."""
        if getattr(self, "vae_decoder", None) is not None:
            return True
        path = self._decoder_checkpoint()
        if path is None:
            return False
        if os.path.isdir(path):
            files = [os.path.join(path, fn) for fn in ("model.safetensors", "diffusion_pytorch_model.safetensors")]
            path = next((f for f in files if os.path.exists(f)), None)
            if path is None:
                return False
        cache = self.__dict__.setdefault("_decodable_cache", {})
        if path not in cache:
            from safetensors import safe_open
            from .vae import CogVideoXVaeDecoder
            try:
                with safe_open(path, "pt") as f:
                    keys = list(f.keys())
            except Exception:                                    # not a safetensors file: nothing this decoder can load
                keys = []
            cache[path] = any(k.startswith(tuple(p + "up." for p in CogVideoXVaeDecoder._PREFIXES + ("",))) for k in keys)
        return cache[path]

    def _decoder(self):
        """the VAE decoder, built on the first call from the ``first_stage_config`` directory the encoder came from"""
        dec = getattr(self, "vae_decoder", None)
        if dec is not None:
            return dec
        import os
        from .vae import CogVideoXVaeDecoder
        node = self._first_stage_config
        params = dict((node.get("params") or {}) if isinstance(node, dict) else {})
        root = params.get("pretrained_model_name_or_path") or params.get("path")
        path = os.path.join(root, params.get("subfolder") or "") if root else None
        if path is None or not os.path.exists(path):
            raise RuntimeError("decoding needs the VAE decoder's weights (the in-tree twin's keys under `decoder.`: decoder.conv_in.conv.weight, "
                               f"decoder.up.N.block.M...), but first_stage_config names no local checkpoint ({path})")
        dec = CogVideoXVaeDecoder.from_pretrained(**params)          # RuntimeError when the file holds no `decoder.` keys
        self.vae_decoder = dec.to(self.device)
        return self.vae_decoder

    @torch.no_grad()
    def decode_first_stage(self, z):
        """z [B, C, F, H, W] scaled latents -> ``vae.decode(z / scaling_factor)`` (an object with ``.sample``), cogvideo_pl.py:162-172"""
        dec = self._decoder()
        return dec.decode(1.0 / dec.config.scaling_factor * z)

    @torch.no_grad()
    def decode_latents(self, latents: torch.Tensor) -> torch.Tensor:
        """latents [B, F, C, H, W] -> frames [B, 3, T, H, W] bf16 (cogvideo_pl.py:410-418 without moving the DiT off the device)"""
        dec = self._decoder()
        latents = latents.permute(0, 2, 1, 3, 4)
        latents = 1 / dec.config.scaling_factor * latents
        return dec.decode(latents.to(dec.dtype)).sample

    def inject_adapter(self, adapter_config):
        self.model.requires_grad_(False)
        cfg = instantiate_from_config(adapter_config) if not isinstance(adapter_config, LoraConfig) else adapter_config
        self.model = get_peft_model(self.model, cfg)
        self.model.print_trainable_parameters()

    def configure_optimizers(self, gradient_clip_val=None, gradient_clip_algorithm="norm"):
        """gradient_clip_val / gradient_clip_algorithm: Lightning's trainer options (config.trainer_options reads them from a recipe)"""
        params = [p for p in self.model.parameters() if p.requires_grad]
        st = getattr(self.model, "_lora_state", None)
        ft = getattr(self.model, "fullft", None)
        if st is None and ft is None and any(p.dtype != torch.float32 for p in params):
            from .fullft import enable_full_finetune        # reference `-fullft` recipes: no adapter_config, all weights train
            ft = enable_full_finetune(self.model)
            params = ft.params
        return FusedAdamW(params, lr=self.learning_rate, lora_state=st, fullft_state=ft, gradient_clip_val=gradient_clip_val,
                          gradient_clip_algorithm=gradient_clip_algorithm)

    def on_save_checkpoint(self, checkpoint: Dict[str, Any]) -> Dict[str, Any]:
        sd = {k: v for k, v in checkpoint["state_dict"].items() if "lora" in k}
        if len(sd) > 0:
            checkpoint["state_dict"] = sd
        return checkpoint

    def on_load_checkpoint(self, checkpoint):
        pass

    # ---- batch handling ----
    def get_batch_input(self, batch):
        if "latents" in batch:
            return {"videos": batch["latents"], "prompt_embeds": batch["prompt_embeds"]}
        if self.first_stage is None or self.cond_stage is None:
            raise RuntimeError("batch has the reference schema {'video','caption'} but no frozen VAE / T5 encoder was given: "
                               "they are outside this engine's hot path (SURVEY 8(f)); pass pre-encoded "
                               "{'latents','prompt_embeds'} or construct the workflow with first_stage=/cond_stage= callables")
        with torch.no_grad():
            ec = self.encoding_cache
            vae = getattr(self, "vae", None)
            if ec is not None and "index" in batch and vae is not None:
                vids = ec.latents(batch["index"], batch["video"], lambda v: vae.encode(v).latent_dist, vae.config.scaling_factor)
            else:
                vids = torch.cat([self.first_stage(v) for v in batch["video"]], dim=0)
            caps = [c for c in batch["caption"]]
            emb = ec.prompt_embeds(caps, self.cond_stage) if ec is not None else self.cond_stage(caps)
        return {"videos": vids, "prompt_embeds": emb}

    def encode_raw_batch(self, batch):
        """reference-schema batch -> {"latents", "prompt_embeds"}: the callable to give vt355.prefetch.EncoderPrefetcher"""
        b = self.get_batch_input(batch)
        return {"latents": b["videos"], "prompt_embeds": b["prompt_embeds"]}

    def training_step(self, batch, batch_idx=0):
        b = self.get_batch_input(batch)
        # [B,C,F,H,W] -> [B,F,C,H,W] (cogvideo_pl.py:817-819); the diffusion math runs in fp32, the DiT in bf16
        x0 = b["videos"].permute(0, 2, 1, 3, 4).to(torch.float32).contiguous()
        prompt_embeds = b["prompt_embeds"]
        B = x0.shape[0]
        noise = torch.randn_like(x0)
        timesteps = torch.randint(0, self.scheduler.config.num_train_timesteps, (B,), device=x0.device).long()
        return self.loss_from(x0, prompt_embeds, noise, timesteps)

    def _prepare_rotary_positional_embeddings(self, height: int, width: int, num_frames: int,
                                              vae_scale_factor_spatial: int = 8, patch_size: int = 2,
                                              attention_head_dim: int = 64, device=None, base_height: int = 480,
                                              base_width: int = 720):
        """(freqs_cos, freqs_sin) for pixel height/width and latent frame count (cogvideo_pl.py:442-473); cached."""
        key = (height, width, num_frames, vae_scale_factor_spatial, patch_size, attention_head_dim, str(device),
               base_height, base_width)
        if key not in self._rope_cache:
            self._rope_cache[key] = prepare_rotary_positional_embeddings(
                height, width, num_frames, vae_scale_factor_spatial, patch_size, attention_head_dim, device,
                base_height, base_width)
        return self._rope_cache[key]

    def loss_from(self, x0, prompt_embeds, noise, timesteps, image_latents=None):
        """Deterministic core of training_step (fixed noise / t) -- what the parity tests call.
        image_latents [B,F,C,H,W] (I2V): concatenated to the noisy latents along the channel axis (cogvideo_i2v.py:158)."""
        noisy = self.scheduler.add_noise(x0, noise, timesteps)
        cfg = getattr(self.model, "config", None) or self.model.base_model.config
        image_rotary_emb = None
        if cfg.use_rotary_positional_embeddings:        # cogvideo_pl.py:846-859
            _, num_frames, _, height, width = x0.shape
            image_rotary_emb = self._prepare_rotary_positional_embeddings(
                height=height * self.vae_scale_factor_spatial, width=width * self.vae_scale_factor_spatial,
                num_frames=num_frames, vae_scale_factor_spatial=self.vae_scale_factor_spatial,
                patch_size=cfg.patch_size, attention_head_dim=cfg.attention_head_dim, device=x0.device)
        model_in = noisy if image_latents is None else torch.cat([noisy, image_latents.to(noisy.dtype)], dim=2)
        out = self.model(hidden_states=model_in, encoder_hidden_states=prompt_embeds, timestep=timesteps,
                         image_rotary_emb=image_rotary_emb, return_dict=False)[0]
        sa, sb, w = self.scheduler.coefficients(timesteps)
        return _LossFn.apply(out, noisy, x0, sa, sb, w)

    # ---- sampling (cogvideo_pl.py:476-772) ----
    _CALLBACK_TENSORS = ("latents", "prompt_embeds", "negative_prompt_embeds", "noise_pred", "old_pred_original_sample",
                         "guidance_scale")

    def _encode_prompts(self, prompt, negative_prompt, do_cfg, num_videos_per_prompt, prompt_embeds, negative_prompt_embeds):
        """(prompt_embeds, negative_prompt_embeds | None) as bf16 device tensors [B * num_videos_per_prompt, L, D] (encode_prompt,
        cogvideo_pl.py:288-367): given embeddings pass through, prompts go through ``cond_stage``"""
        def encode(texts, what):
            if self.cond_stage is None:
                raise RuntimeError(f"sample: {what} needs the T5 text encoder, which this workflow was built without (no local weights); "
                                   f"pass prompt_embeds / negative_prompt_embeds instead")
            return self.cond_stage(list(texts))

        if prompt_embeds is None:
            if prompt is None:
                raise ValueError("sample: give `prompt` or `prompt_embeds`")
            prompt = [prompt] if isinstance(prompt, str) else list(prompt)
            prompt_embeds = encode(prompt, "a text prompt")
        B = prompt_embeds.shape[0]
        if do_cfg and negative_prompt_embeds is None:
            negative_prompt = "" if negative_prompt is None else negative_prompt
            neg = B * [negative_prompt] if isinstance(negative_prompt, str) else list(negative_prompt)
            if len(neg) != B:
                raise ValueError(f"sample: {len(neg)} negative prompts for {B} prompts")
            negative_prompt_embeds = encode(neg, "the negative prompt (guidance_scale > 1)")

        def place(e):
            e = e.to(device=self.device, dtype=torch.bfloat16)
            return e.repeat_interleave(num_videos_per_prompt, dim=0) if num_videos_per_prompt != 1 else e

        return place(prompt_embeds), (place(negative_prompt_embeds) if do_cfg else None)

    def sample(self, prompt=None, negative_prompt=None, height: int = 480, width: int = 720, num_frames: int = 49,
               num_inference_steps: int = 50, timesteps=None, guidance_scale: float = 6, use_dynamic_cfg: bool = False,
               num_videos_per_prompt: int = 1, eta: float = 0.0, generator=None, latents=None, prompt_embeds=None,
               negative_prompt_embeds=None, output_type: str = "pil", sample_precision=None, callback_on_step_end=None,
               callback_on_step_end_tensor_inputs=("latents",), max_sequence_length: int = 226, progress_bar: bool = False,
               seed: Optional[int] = None, **unused):
        """The reference's sampling loop on the device: one DiT forward (both guidance halves in one batch) and one fused
        guidance + DPM-Solver++ kernel per step.  Noise: with ``generator`` torch.randn(generator=...) feeds the kernel; otherwise the
        initial latents and every step's noise are Philox(seed) under the header's noise convention, no torch generator is touched,
        and ``self.last_sample_seed`` holds the seed (8 bytes of os.urandom when ``seed`` is None).  Returns ``video[None].cpu()``:
        [1, B, 3, T, H, W] frames, or [1, B, F, C, H/8, W/8] latents for output_type="latent"."""
        if timesteps is not None:
            raise ValueError("sample: custom `timesteps` are not supported: CogVideoXDPMScheduler.set_timesteps takes none "
                             "(diffusers retrieve_timesteps raises the same way)")
        if sample_precision not in (None, "bfloat16"):
            raise ValueError(f"sample_precision = {sample_precision!r}: this engine samples in bfloat16 only")
        bad = [k for k in callback_on_step_end_tensor_inputs if k not in self._CALLBACK_TENSORS]
        if bad:
            raise ValueError(f"callback_on_step_end_tensor_inputs {bad}: expected names among {self._CALLBACK_TENSORS}")
        was_training = self.model.training
        self.model.eval()
        # a workflow without adapters whose optimizer does not exist yet has trainable base weights and no training state, which the
        # engine refuses to pack; inference needs neither: freeze for the run, then put the flags back and drop that pack
        thawed = []
        if getattr(self.model, "_lora_state", None) is None and getattr(self.model, "fullft", None) is None:
            thawed = [p for p in self.model.parameters() if p.requires_grad]
            for p in thawed:
                p.requires_grad_(False)
        try:
            with torch.no_grad():
                return self._sample(prompt, negative_prompt, height, width, num_frames, int(num_inference_steps), float(guidance_scale),
                                    use_dynamic_cfg, num_videos_per_prompt, generator, latents, prompt_embeds, negative_prompt_embeds,
                                    output_type, callback_on_step_end, tuple(callback_on_step_end_tensor_inputs), progress_bar, seed)
        finally:
            self.model.train(was_training)
            for p in thawed:
                p.requires_grad_(True)
            if thawed:
                self.model._packed = None

    def _sample(self, prompt, negative_prompt, height, width, num_frames, num_inference_steps, guidance_scale, use_dynamic_cfg,
                num_videos_per_prompt, generator, latents, prompt_embeds, negative_prompt_embeds, output_type, callback, callback_inputs,
                progress_bar, seed):
        device = self.device
        do_cfg = guidance_scale > 1.0
        prompt_embeds, negative_prompt_embeds = self._encode_prompts(prompt, negative_prompt, do_cfg, num_videos_per_prompt,
                                                                     prompt_embeds, negative_prompt_embeds)
        B = prompt_embeds.shape[0]
        if do_cfg:
            prompt_embeds = torch.cat([negative_prompt_embeds, prompt_embeds], dim=0)          # cogvideo_pl.py:641
        sch = self.scheduler
        sch.set_timesteps(num_inference_steps, device=device)
        t_dev, t_host = sch.timesteps, sch.timesteps.tolist()
        cfg = getattr(self.model, "config", None) or self.model.base_model.config
        shape = (B, (num_frames - 1) // self.vae_scale_factor_temporal + 1, cfg.in_channels,
                 height // self.vae_scale_factor_spatial, width // self.vae_scale_factor_spatial)
        if generator is None:
            if seed is None:
                seed = int.from_bytes(os.urandom(8), "little")
            seed = int(seed) & 0xFFFFFFFFFFFFFFFF
            self.last_sample_seed = seed
        else:
            seed = None
        if latents is not None:
            if tuple(latents.shape) != shape:
                raise ValueError(f"sample: latents of shape {tuple(latents.shape)}, expected {shape}")
            latents = latents.to(device=device, dtype=torch.bfloat16).contiguous()
        elif generator is not None:
            latents = torch.randn(shape, generator=generator, device=generator.device, dtype=torch.bfloat16).to(device)
        else:
            latents = ops.philox_normal(torch.empty(shape, dtype=torch.bfloat16, device=device), seed, 0)
        latents = latents * sch.init_noise_sigma if sch.init_noise_sigma != 1.0 else latents
        rope = None
        if cfg.use_rotary_positional_embeddings:                                                # cogvideo_pl.py:667-679
            rope = self._prepare_rotary_positional_embeddings(
                height=height, width=width, num_frames=shape[1], vae_scale_factor_spatial=self.vae_scale_factor_spatial,
                patch_size=cfg.patch_size, attention_head_dim=cfg.attention_head_dim, device=device)
        old = None
        steps = enumerate(t_host)
        if progress_bar:
            from tqdm import tqdm
            steps = tqdm(steps, desc="Denoising Steps", total=num_inference_steps)
        for i, t in steps:
            model_in = sch.scale_model_input(torch.cat([latents] * 2) if do_cfg else latents, t)
            noise_pred = self.model(hidden_states=model_in, encoder_hidden_states=prompt_embeds, timestep=t_dev[i].expand(model_in.shape[0]),
                                    image_rotary_emb=rope, return_dict=False)[0]
            g = guidance_scale
            if use_dynamic_cfg:
                # the diffusers pipeline's formula, applied to the scale the step uses (cogvideo_pl.py:711-722 assigns it to a name it
                # never reads); t is the timestep, so the base of the fifth power is negative for every step but the last few
                g = 1 + guidance_scale * ((1 - math.cos(math.pi * ((num_inference_steps - t) / num_inference_steps) ** 5.0)) / 2)
            latents, old = sch.step_guided(noise_pred, g if do_cfg else None, old, t, t_host[i - 1] if i > 0 else None, latents,
                                           generator=generator, seed=seed, noise_stream=i + 1)
            if callback is not None:
                have = {"latents": latents, "prompt_embeds": prompt_embeds, "negative_prompt_embeds": negative_prompt_embeds,
                        "noise_pred": noise_pred, "old_pred_original_sample": old, "guidance_scale": g}
                outs = callback(self, i, t_dev[i], {k: have[k] for k in callback_inputs})
                latents = outs.pop("latents", latents)
                prompt_embeds = outs.pop("prompt_embeds", prompt_embeds)
                negative_prompt_embeds = outs.pop("negative_prompt_embeds", negative_prompt_embeds)
        video = latents if output_type == "latent" else self.decode_latents(latents)
        return video[None, ...].cpu()

    @property
    def log_images(self):
        """``log_images(batch, **kwargs)`` (cogvideo_pl.py:890-899), present only when the workflow can turn latents into frames: without
        a local VAE checkpoint that holds ``decoder.`` weights the attribute does not exist (``hasattr`` is False, as before the sampler)"""
        if not self._decodable():
            raise AttributeError("log_images: first_stage_config names no local VAE checkpoint with `decoder.` weights")
        return self._log_images

    @torch.no_grad()
    def _log_images(self, batch, **kwargs):
        """{"gt": batch["video"], "samples": sample(batch["caption"], num_inference_steps=50, sample_precision="bfloat16")}; kwargs may
        set num_inference_steps, guidance_scale, seed, height, width, num_frames; a batch without captions is sampled from its
        ``prompt_embeds`` (and ``negative_prompt_embeds``): the route when no T5 is on the machine"""
        allowed = ("num_inference_steps", "guidance_scale", "seed", "height", "width", "num_frames")
        args = {"num_inference_steps": 50}
        args.update({k: v for k, v in kwargs.items() if k in allowed})
        if "caption" in batch:
            samples = self.sample([c for c in batch["caption"]], sample_precision="bfloat16", **args)
        else:
            samples = self.sample(prompt_embeds=batch["prompt_embeds"], negative_prompt_embeds=batch.get("negative_prompt_embeds"),
                                  sample_precision="bfloat16", **args)
        return {"gt": batch.get("video"), "samples": samples}


class CogVideoXI2V(CogVideoXWorkFlow):
    """Image-to-video finetune workflow (videotuna/models/cogvideo_hf/cogvideo_i2v.py:39-181): the first-frame image
    latent, zero-padded over the remaining latent frames, rides along as 16 extra input channels; the loss is taken
    on the 16 video channels only.  Pre-encoded batch: {"latents" [B,C,F,H,W], "image_latents" [B,C,1,H,W],
    "prompt_embeds"}; the reference schema {"video","image","caption"} needs the user-supplied frozen encoders."""

    def __init__(self, first_stage_config=None, cond_stage_config=None, denoiser_config=None, scheduler_config=None,
                 learning_rate: float = 6e-6, adapter_config=None, noised_image_input: bool = False,
                 noised_image_dropout: float = 0.05, logdir=None, first_stage=None, cond_stage=None):
        super().__init__(first_stage_config, cond_stage_config, denoiser_config, scheduler_config, learning_rate,
                         adapter_config, logdir, first_stage=first_stage, cond_stage=cond_stage)
        self.noised_image_input = noised_image_input
        self.noised_image_dropout = noised_image_dropout

    def sample(self, *args, **kwargs):
        raise NotImplementedError("CogVideoXI2V.sample is not built: the image-to-video loop concatenates the image latents to the "
                                  "model input at every step (cogvideo_i2v.py), which the text-to-video sampler does not do")

    @property
    def log_images(self):
        raise AttributeError("log_images: CogVideoXI2V.sample is not built")

    def get_batch_input(self, batch):
        if "latents" in batch:
            vids, imgs = batch["latents"], batch["image_latents"]
            emb = batch["prompt_embeds"]
        else:
            if self.first_stage is None or self.cond_stage is None:
                raise RuntimeError("batch has the reference schema {'video','image','caption'} but no frozen VAE / T5 encoder "
                                   "was given (outside this engine's hot path, SURVEY 8(f)); pass pre-encoded "
                                   "{'latents','image_latents','prompt_embeds'}")
            with torch.no_grad():
                vids = torch.cat([self.first_stage(v) for v in batch["video"]], dim=0)
                # reference schema: image [3,1,H,W] (cogvideo_i2v.py:65-68); a plain [3,H,W] frame gets its time axis here
                imgs = torch.cat([self.first_stage(im.unsqueeze(1) if im.dim() == 3 else im) for im in batch["image"]], dim=0)
                emb = self.cond_stage([c for c in batch["caption"]])
        vids = vids.permute(0, 2, 1, 3, 4).contiguous()           # [B,C,T,H,W] -> [B,T,C,H,W]
        imgs = imgs.permute(0, 2, 1, 3, 4).contiguous()
        pad = vids.new_zeros((vids.shape[0], vids.shape[1] - imgs.shape[1], *vids.shape[2:]))
        imgs = torch.cat([imgs.to(vids.dtype), pad], dim=1)       # image latent in frame 0, zeros after (i2v.py:89-96)
        import random
        if random.random() < self.noised_image_dropout:           # conditional image dropout (i2v.py:98-99)
            imgs = torch.zeros_like(imgs)
        return {"videos": vids, "images": imgs, "prompt_embeds": emb}

    def training_step(self, batch, batch_idx=0):
        b = self.get_batch_input(batch)
        x0 = b["videos"].to(torch.float32).contiguous()
        B = x0.shape[0]
        noise = torch.randn_like(x0)
        timesteps = torch.randint(0, self.scheduler.config.num_train_timesteps, (B,), device=x0.device).long()
        return self.loss_from(x0, b["prompt_embeds"], noise, timesteps, image_latents=b["images"].to(torch.float32))
