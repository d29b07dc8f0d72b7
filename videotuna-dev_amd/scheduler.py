"""Noise schedule with the surface of ``diffusers.CogVideoXDPMScheduler`` that training touches
(cogvideo_pl.py:838-877): ``config.num_train_timesteps``, ``alphas_cumprod``, ``add_noise``, ``get_velocity``, and the one
sampling touches (cogvideo_pl.py:644-746): ``set_timesteps``, ``timesteps``, ``scale_model_input``, ``init_noise_sigma``, ``order``,
``step``.

abar_t: scaled-linear betas (0.00085 -> 0.012, 1000 steps, fp64) -> cumprod -> SNR shift
abar/(s + (1-s) abar) with s = snr_shift_scale (3.0 for CogVideoX-2b) -> zero-terminal-SNR rescale.
In-tree twin: videotuna/models/cogvideo_sat/sgm/modules/diffusionmodules/discretizer.py:80-140 (pinned by
tests/golden/schedule_cogvideox.npz).  The values of the real checkpoint's scheduler_config.json are not available
offline, so they are explicit constructor arguments here.
"""
from __future__ import annotations

import json
import math
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import ops


class CogVideoXDPMScheduler:
    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "scaled_linear", snr_shift_scale: float = 3.0, rescale_betas_zero_snr: bool = True,
                 prediction_type: str = "v_prediction", timestep_spacing: str = "leading", steps_offset: int = 0,
                 set_alpha_to_one: bool = True, **unused):
        if beta_schedule != "scaled_linear":
            raise NotImplementedError(beta_schedule)
        if timestep_spacing not in ("leading", "linspace", "trailing"):
            raise ValueError(f"timestep_spacing {timestep_spacing!r}: expected 'leading', 'linspace' or 'trailing'")
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, snr_shift_scale=snr_shift_scale,
                                      rescale_betas_zero_snr=rescale_betas_zero_snr, prediction_type=prediction_type,
                                      timestep_spacing=timestep_spacing, steps_offset=int(steps_offset),
                                      set_alpha_to_one=bool(set_alpha_to_one))
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float64) ** 2
        ac = torch.cumprod(1.0 - betas, dim=0)
        ac = ac / (snr_shift_scale + (1.0 - snr_shift_scale) * ac)
        if rescale_betas_zero_snr:
            s = ac.sqrt()
            s0, sT = s[0].clone(), s[-1].clone()
            s = (s - sT) * (s0 / (s0 - sT))
            ac = s ** 2
        self.alphas_cumprod = ac                      # fp64, CPU (like diffusers); device copies are cached
        self._dev = {}
        # ---- inference surface ----
        self.final_alpha_cumprod = torch.tensor(1.0, dtype=torch.float64) if set_alpha_to_one else ac[0].clone()
        self.init_noise_sigma = 1.0
        self.order = 1
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder=None, **kw):
        root = os.path.join(pretrained_model_name_or_path, subfolder) if subfolder else pretrained_model_name_or_path
        with open(os.path.join(root, "scheduler_config.json")) as f:
            return cls(**{k: v for k, v in json.load(f).items() if not k.startswith("_")})

    def coefficients(self, timesteps: torch.Tensor):
        """(sqrt(abar_t), sqrt(1-abar_t), 1/(1-abar_t)) as fp32 device vectors [B]."""
        dev = timesteps.device
        if dev not in self._dev:
            a = self.alphas_cumprod
            tab = torch.stack([a.sqrt(), (1 - a).sqrt(), 1 / (1 - a)]).to(torch.float32).to(dev)
            self._dev[dev] = tab
        tab = self._dev[dev]
        sel = tab[:, timesteps]                      # tiny gather on [3, B]
        return sel[0].contiguous(), sel[1].contiguous(), sel[2].contiguous()

    def add_noise(self, original_samples, noise, timesteps):
        """fp32 x0 / noise in, bf16 noisy sample out (HIP kernel)."""
        sa, sb, _ = self.coefficients(timesteps)
        out = torch.empty(original_samples.shape, dtype=torch.bfloat16, device=original_samples.device)
        ops.add_noise(original_samples.contiguous(), noise.contiguous(), sa, sb, out)
        return out

    # ---- sampling: diffusers CogVideoXDPMScheduler.set_timesteps / step (DPM-Solver++ 2M in its SDE form, v-prediction) ----
    def scale_model_input(self, sample, timestep=None):
        return sample

    def set_timesteps(self, num_inference_steps: int, device=None):
        N, n = self.config.num_train_timesteps, int(num_inference_steps)
        if not 1 <= n <= N:
            raise ValueError(f"num_inference_steps = {num_inference_steps} must lie in 1..{N} (num_train_timesteps)")
        self.num_inference_steps = n
        self.timesteps = torch.from_numpy(spaced_timesteps(N, n, self.config.timestep_spacing, self.config.steps_offset)).to(device)

    def step_coefficients(self, timestep, timestep_back=None, have_old: bool = True):
        """the host scalars of one step, fp64 from the fp64 table: dict(sa, sb, m1, m2, m3, m4, m_noise, second_order, prev_timestep).
        Only finite numbers leave: a second-order step whose m3 / m4 are not finite raises (the last step, abar_prev = 1, must be -- and
        by the prev_timestep < 0 rule is -- first order)."""
        if self.num_inference_steps is None:
            raise ValueError("number of inference steps is None: run set_timesteps first")
        N, t = self.config.num_train_timesteps, int(timestep)
        prev_t = t - N // self.num_inference_steps
        ac = self.alphas_cumprod
        a_t = ac[t].item()
        a_prev = ac[prev_t].item() if prev_t >= 0 else float(self.final_alpha_cumprod)
        second = bool(have_old) and prev_t >= 0
        if second and timestep_back is None:
            raise ValueError("a second-order step needs timestep_back, the timestep old_pred_original_sample was predicted at")
        a_back = ac[int(timestep_back)].item() if second else None
        c = dpm_coefficients(a_t, a_prev, a_back)
        c.update(sa=math.sqrt(a_t), sb=math.sqrt(1.0 - a_t), second_order=second, prev_timestep=prev_t)
        names = ("sa", "sb", "m1", "m2", "m_noise") + (("m3", "m4") if second else ())
        bad = {k: c[k] for k in names if not math.isfinite(c[k])}
        if bad:
            raise ValueError(f"step at t = {t} (prev {prev_t}, back {timestep_back}): non-finite coefficients {bad}")
        if not second:
            c["m3"], c["m4"] = 0.0, 0.0
        return c

    def step(self, model_output, old_pred_original_sample, timestep, timestep_back, sample, eta: float = 0.0, generator=None,
             variance_noise=None, return_dict: bool = False):
        """(prev_sample bf16, pred_original_sample fp32) from an already guided model_output [B, ...] (HIP kernel; the workflow's loop
        hands the kernel both guidance halves instead, ``step_guided``)."""
        return self.step_guided(model_output, None, old_pred_original_sample, timestep, timestep_back, sample, generator=generator,
                                variance_noise=variance_noise)

    def step_guided(self, model_output, guidance_scale, old_pred_original_sample, timestep, timestep_back, sample, generator=None,
                    variance_noise=None, seed=None, noise_stream: int = 0):
        """model_output [2B, ...] = (uncond, cond) with a guidance_scale, or [B, ...] with None.  Noise: variance_noise, else
        torch.randn(generator=) when ``seed`` is None, else drawn in the kernel as Philox(seed, noise_stream) (no torch generator)."""
        c = self.step_coefficients(timestep, timestep_back, old_pred_original_sample is not None)
        x = sample.to(torch.bfloat16).contiguous()
        v = model_output.to(torch.bfloat16).contiguous()
        noise = None
        if c["m_noise"] != 0.0:
            if variance_noise is not None:
                noise = variance_noise.to(torch.float32).contiguous()
            elif seed is None:
                gdev = x.device if generator is None else generator.device
                noise = torch.randn(x.shape, generator=generator, device=gdev, dtype=torch.float32).to(x.device)
        old = old_pred_original_sample if c["second_order"] else None
        if old is not None:
            old = old.to(torch.float32).contiguous()
        x_out = torch.empty_like(x)
        x0 = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        ops.dpm_step(v, x, old, noise, x_out, x0, guidance_scale, c["sa"], c["sb"], c["m1"], c["m2"], c["m3"], c["m4"], c["m_noise"],
                     c["second_order"], seed=seed or 0, stream_id=noise_stream)
        return x_out, x0


def spaced_timesteps(N: int, n: int, spacing: str, steps_offset: int = 0) -> np.ndarray:
    """the int64 timestep list of diffusers' set_timesteps for the three spacing modes"""
    if spacing == "leading":
        return (np.arange(0, n) * (N // n)).round()[::-1].copy().astype(np.int64) + steps_offset
    if spacing == "linspace":
        return np.linspace(0, N - 1, n).round()[::-1].copy().astype(np.int64)
    if spacing == "trailing":
        return np.round(np.arange(N, 0, -N / n)).astype(np.int64) - 1
    raise ValueError(f"timestep_spacing {spacing!r}")


def dpm_coefficients(a_t: float, a_prev: float, a_back=None) -> dict:
    """m1, m2, m_noise (and m3, m4 with a_back) of CogVideoXDPMScheduler.step from the three cumulative alphas, in fp64; abar = 0 and
    abar = 1 give infinite log-SNRs and finite m1 / m2 / m_noise.  In-tree twin: VPSDEDPMPP2MSampler.get_variables / get_mult
    (cogvideo_sat/sgm/modules/diffusionmodules/sampling.py:763-804)."""
    a_t, a_prev = np.float64(a_t), np.float64(a_prev)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lam = lambda a: np.log(np.sqrt(a / (1.0 - a)))          # noqa: E731
        lam_t, lam_prev = lam(a_t), lam(a_prev)
        h = lam_prev - lam_t
        out = {"h": float(h),
               "m1": float(np.sqrt((1.0 - a_prev) / (1.0 - a_t)) * np.exp(-h)),
               "m2": float(np.expm1(-2.0 * h) * np.sqrt(a_prev)),
               "m_noise": float(np.sqrt(1.0 - a_prev) * np.sqrt(1.0 - np.exp(-2.0 * h)))}
        if a_back is not None:
            r = (lam_t - lam(np.float64(a_back))) / h
            out.update(r=float(r), m3=float(1.0 + 1.0 / (2.0 * r)), m4=float(1.0 / (2.0 * r)))
    return out
