#!/usr/bin/env python3
"""Kernel bench of the sampler's two kernels at CogVideoX's latent size (13 x 16 x 60 x 90 elements per sample), and one whole
`sample()` of the CogVideoX-2B architecture (seeded weights, given prompt embeddings) with its time split and peak HBM.

One process; the candidates of a line are launched ALTERNATELY, 20 timed launches each after a warm-up, device events around each
launch; the figures are the median and the spread (max - min) of the 20.  Needs a GPU: there is no fallback.

  vt_dpm_step, noise fed / drawn in the kernel    guidance combine + DPM-Solver++ step in one launch
  unfused torch                                   the same step as the torch expression (chunk, guidance, x0, d, x', casts) on the device
  vt_philox_normal / torch.randn                  fp32 noise of one step; bf16 initial latents

Usage: python tools/kbench_sampler.py [--out profiles/sampler_kbench.txt] [--launches 20] [--no-sample] [--steps 50]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vt355 import ops  # noqa: E402

BF16 = torch.bfloat16
PER = 13 * 16 * 60 * 90


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return statistics.median(ms), max(ms) - min(ms)


def alternate(fns, n):
    for f in fns:
        f(); f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(n):
        for k, f in enumerate(fns):
            ts[k].append(timed(f))
    return [stats(t) for t in ts]


def bench_step(B, n, dev, log):
    g = torch.Generator(device=dev).manual_seed(B)
    v = torch.randn(2 * B, PER, generator=g, device=dev).to(BF16)
    x = torch.randn(B, PER, generator=g, device=dev).to(BF16)
    old = torch.randn(B, PER, generator=g, device=dev)
    noise = torch.randn(B, PER, generator=g, device=dev)
    xo, x0 = torch.empty_like(x), torch.empty_like(old)
    sa, sb, m1, m2, m3, m4, mn, gs = 0.31, 0.95, 0.334, -0.522, 1.398, 0.398, 0.713, 6.0

    def fed():
        ops.dpm_step(v, x, old, noise, xo, x0, gs, sa, sb, m1, m2, m3, m4, mn, True)

    def drawn():
        ops.dpm_step(v, x, old, None, xo, x0, gs, sa, sb, m1, m2, m3, m4, mn, True, seed=7, stream_id=3)

    def unfused():
        vu, vc = v.chunk(2)
        vv = vu + gs * (vc - vu)
        p0 = sa * x.float() - sb * vv.float()
        d = m3 * p0 - m4 * old
        return (m1 * x.float() - m2 * d + mn * noise).to(BF16), p0

    def unfused_randn():
        vu, vc = v.chunk(2)
        vv = vu + gs * (vc - vu)
        p0 = sa * x.float() - sb * vv.float()
        d = m3 * p0 - m4 * old
        return (m1 * x.float() - m2 * d + mn * torch.randn_like(old)).to(BF16), p0

    (mf, sf), (md, sd), (mu, su), (mr, sr) = alternate([fed, drawn, unfused, unfused_randn], n)
    nbytes = B * PER * (2 * 2 + 2 + 4 + 4 + 2 + 4)
    log(f"dpm step B={B} per={PER} ({nbytes / 1e6:.1f} MB with fed noise)")
    log(f"    vt_dpm_step, noise fed         median {mf * 1e3:8.1f} us  spread {sf * 1e3:7.1f} us  {nbytes / mf / 1e9:6.2f} TB/s")
    log(f"    vt_dpm_step, noise in kernel   median {md * 1e3:8.1f} us  spread {sd * 1e3:7.1f} us")
    log(f"    unfused torch, noise given     median {mu * 1e3:8.1f} us  spread {su * 1e3:7.1f} us  = {mu / mf:5.1f} x the fed kernel")
    log(f"    unfused torch + torch.randn    median {mr * 1e3:8.1f} us  spread {sr * 1e3:7.1f} us  = {mr / md:5.1f} x the drawing kernel")

    f32, b16 = torch.empty(B, PER, device=dev), torch.empty(B, PER, dtype=BF16, device=dev)
    (p32, s32), (t32, u32), (p16, s16), (t16, u16) = alternate(
        [lambda: ops.philox_normal(f32, 7, 1), lambda: torch.randn(B, PER, device=dev),
         lambda: ops.philox_normal(b16, 7, 0), lambda: torch.randn(B, PER, device=dev, dtype=BF16)], n)
    log(f"    vt_philox_normal fp32          median {p32 * 1e3:8.1f} us  spread {s32 * 1e3:7.1f} us;  torch.randn fp32 median {t32 * 1e3:8.1f} us  spread {u32 * 1e3:7.1f} us  "
        f"(ratio {p32 / t32:.2f})")
    log(f"    vt_philox_normal bf16          median {p16 * 1e3:8.1f} us  spread {s16 * 1e3:7.1f} us;  torch.randn bf16 median {t16 * 1e3:8.1f} us  spread {u16 * 1e3:7.1f} us  "
        f"(ratio {p16 / t16:.2f})")


def whole_sample(steps, dev, log):
    from vt355.vae import CogVideoXVaeDecoder
    from vt355.workflow import CogVideoXWorkFlow
    wf = CogVideoXWorkFlow(denoiser_config={"target": "vt355.dit.CogVideoXTransformer3DModel"},
                           scheduler_config={"target": "vt355.scheduler.CogVideoXDPMScheduler", "params": {"timestep_spacing": "trailing"}})
    wf.to(dev)
    gen = torch.Generator(device=dev).manual_seed(1234)
    with torch.no_grad():                                          # the benchmark's seeded initialisation
        for name, p in wf.model.named_parameters():
            p.normal_(0.0, 0.02, generator=gen)
            if name.endswith(("norm.weight", "norm_final.weight", "norm_q.weight", "norm_k.weight")):
                p.add_(1.0)
    wf.vae_decoder = CogVideoXVaeDecoder().init_weights(1).to(dev)
    pe = (torch.randn(1, 226, 4096, generator=gen, device=dev) * 0.5).to(BF16)
    ne = (torch.randn(1, 226, 4096, generator=gen, device=dev) * 0.5).to(BF16)
    spans = {"dit": [], "step": [], "decode": []}

    def span(name, fn):
        def wrapped(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); out = fn(*a, **k); e1.record()
            spans[name].append((e0, e1))
            return out
        return wrapped

    wf.model.forward = span("dit", wf.model.forward)
    wf.scheduler.step_guided = span("step", wf.scheduler.step_guided)
    wf.decode_latents = span("decode", wf.decode_latents)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, guidance_scale=6, seed=1)
    wf.sample(num_inference_steps=2, **kw)                         # warm-up: every shape of the timed run
    torch.cuda.synchronize()
    for v in spans.values():
        v.clear()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    video = wf.sample(num_inference_steps=steps, **kw)             # ends in a device-to-host copy: the clock covers all device work
    wall = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated()
    tot = {k: sum(a.elapsed_time(b) for a, b in v) / 1e3 for k, v in spans.items()}
    finite = bool(torch.isfinite(video.float()).all())
    log(f"sample() CogVideoX-2B architecture, 49x480x720, {steps} steps, guidance 6, B=1, seeded weights, prompt_embeds given, Philox noise:")
    log(f"    {wall:.2f} s per video (host clock, including the copy of {tuple(video.shape)} frames to the host; output finite: {finite})")
    log(f"    DiT forwards (batch 2) {tot['dit']:.2f} s in {len(spans['dit'])} calls ({tot['dit'] / max(1, len(spans['dit'])) * 1e3:.1f} ms each), "
        f"step kernels {tot['step'] * 1e3:.2f} ms in {len(spans['step'])} calls (host coefficients + launch), decode {tot['decode'] * 1e3:.1f} ms")
    log(f"    peak HBM {peak / 1e9:.2f} GB allocated ({base / 1e9:.2f} GB of it weights and packed copies)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_kbench.txt"))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--no-sample", action="store_true", help="kernels only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_sampler needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"# tools/kbench_sampler.py on {torch.cuda.get_device_name(0)}: median and spread (max - min) of {a.launches} alternating launches per candidate")
    for B in (1, 2):
        bench_step(B, a.launches, dev, log)
    torch.cuda.empty_cache()
    if not a.no_sample:
        whole_sample(a.steps, dev, log)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
