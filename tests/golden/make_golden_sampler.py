#!/usr/bin/env python3
"""Generates tests/golden/dpm_sampler.npz by running the reference's own VPSDEDPMPP2MSampler (the in-tree twin of diffusers'
CogVideoXDPMScheduler.step: videotuna/models/cogvideo_sat/sgm/modules/diffusionmodules/sampling.py:762-869) in the build container, under
stubs for omegaconf, the sgm package skeleton, sgm.util (append_dims as the reference defines it), sampling_utils and guiders.

Recorded:
  * get_variables / get_mult / mult_noise in fp64 for every step of the 50-step and the 4-step trailing schedules over the cumulative
    alphas of schedule_cogvideox.npz (shift 3), each step with the neighbours the diffusers rules give it (prev = t - N // n, abar 1 past
    the end; back = the previous list entry), and for three edge rows (abar 0 -> 0.3, 0.3 -> 0.9 behind an abar = 0 step, 0.9 -> 1.0);
  * one sampler_step trajectory (three transitions, fp32) on a tiny tensor with a linear stub denoiser and recorded noise.
The timestep lists themselves have no importable reference (diffusers is absent): the fixture's metadata marks them
"self-oracle, reference-unpinned", as the CogVideoX fixtures are.
Run:  python tests/golden/make_golden_sampler.py   (needs /root/reference; the .npz file it writes is what travels)"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import sampler_ref as R  # noqa: E402


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    m.__path__ = []
    sys.modules[name] = m
    return m


def load_twin():
    stub("omegaconf", ListConfig=list, OmegaConf=dict)
    for pkg in ("sgm", "sgm.modules", "sgm.modules.diffusionmodules"):
        stub(pkg)
    stub("sgm.modules.diffusionmodules.sampling_utils", get_ancestral_step=None, linear_multistep_coeff=None, to_d=None,
         to_neg_log_sigma=None, to_sigma=None)
    stub("sgm.util", append_dims=lambda x, target: x[(...,) + (None,) * (target - x.ndim)], default=lambda v, d: d if v is None else v,
         instantiate_from_config=None)
    stub("sgm.modules.diffusionmodules.guiders", DynamicCFG=type("DynamicCFG", (), {}))
    name = "sgm.modules.diffusionmodules.sampling"
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, "videotuna/models/cogvideo_sat/sgm/modules/diffusionmodules/sampling.py"))
    mod = importlib.util.module_from_spec(spec)
    mod.__package__ = "sgm.modules.diffusionmodules"
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def scalars(S, a_t, a_prev, a_back):
    """[h, r, m1, m2, m3, m4, m_noise] of the twin in fp64 (nan where the twin gives none)"""
    s = lambda a: None if a is None else torch.tensor(a, dtype=torch.float64).sqrt()       # noqa: E731
    st, sp, sb = s(a_t), s(a_prev), s(a_back)
    h, r, _, _ = S.get_variables(st, sp, sb)
    mult = S.get_mult(h, r, st, sp, sb)
    mn = (1 - sp ** 2) ** 0.5 * (1 - (-2 * h).exp()) ** 0.5
    f = lambda v: float("nan") if v is None else float(v)                                   # noqa: E731
    return [f(h), f(r), f(mult[0]), f(mult[1]), f(mult[2]) if sb is not None else float("nan"),
            f(mult[3]) if sb is not None else float("nan"), f(mn)]


def main():
    mod = load_twin()
    S = mod.VPSDEDPMPP2MSampler.__new__(mod.VPSDEDPMPP2MSampler)
    g = np.load(os.path.join(HERE, "schedule_cogvideox.npz"))
    abar = g["sqrt_abar_shift3"].astype(np.float64) ** 2            # the twin's own table (fp32 sqrt(abar), t ascending), squared in fp64
    N = abar.shape[0]
    rec = {"abar": abar}
    for n in (50, 4):
        ts = R.timesteps(N, n, "trailing")
        rows = []
        for i, t in enumerate(ts):
            prev = t - N // n
            a_prev = abar[prev] if prev >= 0 else 1.0
            second = i > 0 and prev >= 0
            rows.append(scalars(S, abar[t], a_prev, abar[ts[i - 1]] if second else None))
        rec[f"trailing{n}.timesteps"] = np.array(ts, dtype=np.int64)
        rec[f"trailing{n}.scalars"] = np.array(rows, dtype=np.float64)
    rec["edge.abar"] = np.array([[0.0, 0.3, np.nan], [0.3, 0.9, 0.0], [0.9, 1.0, 0.3]])
    rec["edge.scalars"] = np.array([scalars(S, 0.0, 0.3, None), scalars(S, 0.3, 0.9, 0.0), scalars(S, 0.9, 1.0, 0.3)])

    # ---- one trajectory of sampler_step in fp32: 999 -> 749 (first order), 749 -> 499 (behind the abar = 0 step), 499 -> 249
    ts = R.timesteps(N, 4, "trailing")
    gen = torch.Generator().manual_seed(31)
    x = torch.randn(2, 3, 5, generator=gen)
    noise = [torch.randn(2, 3, 5, generator=gen) for _ in range(3)]
    den = R.linear_denoiser(2, guided=False)
    cur = {}

    def denoise(xx, denoiser, alpha_cumprod_sqrt, cond, uc, timestep, idx, **kw):      # v-prediction stub -> the x0 the twin's step takes
        a = alpha_cumprod_sqrt.reshape(-1, 1, 1)
        v = torch.from_numpy(den(xx.double().numpy(), cur["t"])).to(torch.float32)
        return a * xx - (1 - a ** 2) ** 0.5 * v

    S.denoise = denoise
    randn_like = torch.randn_like
    sq = lambda t: torch.full((2,), float(g["sqrt_abar_shift3"][t]), dtype=torch.float32)      # noqa: E731
    traj, old = [], None
    try:
        for i in range(3):
            cur["t"] = ts[i]
            torch.randn_like = lambda t_, i=i: noise[i]            # both draws of a second-order step return the step's recorded noise
            x, old = S.sampler_step(old, sq(ts[i - 1]) if i > 0 else None, sq(ts[i]), sq(ts[i + 1]), None, x, None, idx=None,
                                    timestep=ts[i])
            traj.append(x.clone())
    finally:
        torch.randn_like = randn_like
    rec["traj.x_init"] = torch.randn(2, 3, 5, generator=torch.Generator().manual_seed(31)).numpy()
    rec["traj.noise"] = torch.stack(noise).numpy()
    rec["traj.timesteps"] = np.array(ts, dtype=np.int64)
    rec["traj.x"] = torch.stack(traj).numpy()
    rec["meta"] = np.array(json.dumps({
        "scalars": "columns h, r, m1, m2, m3, m4, m_noise; VPSDEDPMPP2MSampler.get_variables / get_mult / mult_noise in fp64",
        "timesteps": "self-oracle, reference-unpinned (diffusers' set_timesteps is not importable here; restated in tests/sampler_ref.py)",
        "trajectory": "VPSDEDPMPP2MSampler.sampler_step in fp32, tests/sampler_ref.linear_denoiser(2, guided=False) as v(x, t), "
                      "one recorded noise per step"}))
    np.savez(os.path.join(HERE, "dpm_sampler.npz"), **rec)
    print("wrote dpm_sampler.npz", {k: np.asarray(v).shape for k, v in rec.items()})
    print(rec["edge.scalars"])


if __name__ == "__main__":
    main()
