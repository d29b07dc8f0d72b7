"""DynamiCrafter (configs/002_dynamicrafter/dc_i2v_1024.yaml) on the device: step time of the recipe's UNet and an A/B of its one new
kernel.  Prints one JSON line per part.

  kernel   the dual-context cross-attention (csrc/attn_dual.hip: text + per-frame image keys, two softmaxes, one launch) against the only
           other way this engine can compute it: two vt_attn_small launches (text keys; image keys with one item per frame) plus the
           elementwise adds of o and dq -- forward and backward, at the four levels' shapes of 16 x 40 x 64 latents, batch 4.  HIP events,
           the two paths alternate for --rounds rounds; per path the median and the spread (max - min) of the rounds are reported.
  step40   full fine-tune step of the recipe (LatentVisualDiffusionFlow.training_step: condition dropout, Resampler, q_sample, UNet with
           img_cross_attention / fs_condition / 8 input channels / dropout 0.1 in train mode, v-MSE, backward through both modules, fused
           AdamW of both) at latents [4, 4, 16, 40, 64] -- the size and batch of ``bench.py --model vc2``.
  step72   the same at the recipe's own size, latents [2, 8, 16, 72, 128] (576 x 1024 video), batch 2, with the peak memory.
The step parts each run in a child process (a fresh allocator, its own time limit).

    python tools/bench_dc.py [--parts kernel,step40,step72] [--rounds 5] [--steps 4] [--warmup 2] [--timeout 500]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = [(2560, 5), (640, 10), (160, 20), (40, 20)]          # (rows per frame, heads) of the four levels at 40 x 64 latents, 320 / 640 / 1280 ch


def bench_kernel(rounds: int, iters: int):
    sys.path.insert(0, ROOT)
    import torch
    from vt355 import ops
    dev = torch.device("cuda:0")
    BF = torch.bfloat16
    B, T, Sa, Sb = 4, 16, 77, 16
    out = {"metric": "dual-context cross-attention, fused kernel vs two attn_small launches + adds", "unit": "ms", "batch": B, "frames": T,
           "text_keys": Sa, "image_keys": Sb, "rounds": rounds, "iters_per_round": iters, "levels": []}
    for HW, H in LEVELS:
        D, Sq = H * 64, T * HW
        g = torch.Generator(device=dev).manual_seed(HW)
        q = torch.randn(B, Sq, D, device=dev, generator=g).to(BF)
        kv = torch.randn(B, Sa, 2 * D, device=dev, generator=g).to(BF)
        kvi = torch.randn(B * T, Sb, 2 * D, device=dev, generator=g).to(BF)
        do = torch.randn(B, Sq, D, device=dev, generator=g).to(BF)
        o, dq = torch.empty_like(q), torch.empty_like(q)
        lse = torch.empty(2, B, H, Sq, device=dev)
        dk, dv = torch.empty(B, Sa, D, device=dev), torch.empty(B, Sa, D, device=dev)
        dki, dvi = torch.empty(B * T, Sb, D, device=dev), torch.empty(B * T, Sb, D, device=dev)
        need = ops.attn_dual_ws_floats(B, H, Sq, HW, Sa, Sb)
        ws = torch.empty(max(need, 1), device=dev)
        # composition: image attention sees one item per frame
        q_f, do_f = q.view(B * T, HW, D), do.view(B * T, HW, D)
        o2, dq2 = torch.empty_like(q), torch.empty_like(q)
        lse_a, lse_b = torch.empty(B, H, Sq, device=dev), torch.empty(B * T, H, HW, device=dev)

        def fused_fwd():
            ops.attn_dual_fwd(q, kv[..., :D], kv[..., D:], kvi[..., :D], kvi[..., D:], o, lse, H, 0.125, HW, 1.0)

        def fused_bwd():
            ops.attn_dual_bwd(q, kv[..., :D], kv[..., D:], kvi[..., :D], kvi[..., D:], do, lse, dq, dk, dv, dki, dvi, H, 0.125, HW, 1.0, ws=ws)

        def comp_fwd():
            ops.attn_small_fwd(q, kv[..., :D], kv[..., D:], o, lse_a, H, 0.125)
            ops.attn_small_fwd(q_f, kvi[..., :D], kvi[..., D:], o2.view(B * T, HW, D), lse_b, H, 0.125)
            ops.add_rows(o.view(-1, D), o2.view(-1, D), o.view(-1, D))

        def comp_bwd():
            ops.attn_small_bwd(q, kv[..., :D], kv[..., D:], o, do, lse_a, dq, dk, dv, H, 0.125)
            ops.attn_small_bwd(q_f, kvi[..., :D], kvi[..., D:], o2.view(B * T, HW, D), do_f, lse_b, dq2.view(B * T, HW, D), dki, dvi, H, 0.125)
            ops.add_rows(dq.view(-1, D), dq2.view(-1, D), dq.view(-1, D))

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / iters

        fns = {"fused_fwd": fused_fwd, "comp_fwd": comp_fwd, "fused_bwd": fused_bwd, "comp_bwd": comp_bwd}
        comp_fwd(); fused_fwd()                      # lse of both paths exist before any backward is timed
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(rounds):                      # alternate the paths inside every round
            for k, fn in fns.items():
                times[k].append(timed(fn))
        # the composition's own separate pieces would have to keep o of each branch for the backward; the fused path reads no o at all
        byt = lambda reads, writes: (reads + writes) * B * Sq * D * 2 / 1e9
        lv = {"rows_per_frame": HW, "heads": H, "channels": D, "rows": B * Sq, "workspace_mb": round(need * 4 / 1e6, 1)}
        for k, v in times.items():
            lv[k] = {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)}
        for ph, reads, writes in (("fwd", 1, 1), ("bwd", 2, 1)):
            f, c = lv["fused_" + ph], lv["comp_" + ph]
            lv[ph + "_fused_over_comp"] = round(f["median_ms"] / c["median_ms"], 3)
            lv[ph + "_fused_gbps_q_side"] = round(byt(reads, writes) / (f["median_ms"] / 1e3), 1)      # q / dO read + o / dq written once
            lv[ph + "_not_slower_beyond_spread"] = bool(f["median_ms"] <= c["median_ms"] + max(f["spread_ms"], c["spread_ms"]))
        out["levels"].append(lv)
    print(json.dumps(out), flush=True)


def bench_step(latent_hw, B: int, steps: int, warmup: int):
    sys.path.insert(0, ROOT)
    import torch
    from vt355.lvdm import LatentVisualDiffusionFlow
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    BF = torch.bfloat16
    T, (H, W) = 16, latent_hw
    unet = dict(target="vt355.unet.UNetModel", params=dict(
        in_channels=8, out_channels=4, model_channels=320, attention_resolutions=[4, 2, 1], num_res_blocks=2, channel_mult=[1, 2, 4, 4],
        dropout=0.1, num_head_channels=64, transformer_depth=1, context_dim=1024, use_linear=True, use_checkpoint=True,
        temporal_conv=True, temporal_attention=True, temporal_selfatt_only=True, use_relative_position=False,
        use_causal_attention=False, temporal_length=16, addition_attention=True, img_cross_attention=True, default_fs=10, fs_condition=True))
    proj = dict(target="vt355.resampler.Resampler", params=dict(dim=1024, depth=4, dim_head=64, heads=12, num_queries=16, embedding_dim=1280,
                                                                 output_dim=1024, ff_mult=4, video_length=16))
    sched = dict(target="vt355.lvdm.LDDPM", params=dict(timesteps=1000, linear_start=0.00085, linear_end=0.012, rescale_betas_zero_snr=True))
    flow = LatentVisualDiffusionFlow(unet_config=unet, image_proj_stage_config=proj, diffusion_scheduler_config=sched, parameterization="v",
                                     use_scale=True, scale_b=0.3, uncond_prob=0.05, uncond_type="empty_seq", rand_cond_frame=True,
                                     fps_condition_type="fps", image_proj_model_trainable=True, base_learning_rate=1e-5)
    flow.model.init_weights(1234)
    flow.image_proj_model.init_weights(4321)
    flow.to(dev)
    flow.train()
    opt = flow.configure_optimizers()
    g = torch.Generator(device=dev).manual_seed(20230211)
    null_ctx = torch.randn(77, 1024, device=dev, generator=g).to(BF)            # stand for the encodings of "" and of an all-zero image
    null_tok = torch.randn(257, 1280, device=dev, generator=g).to(BF)
    losses = []

    def step():
        opt.zero_grad()
        batch = {"latents": torch.randn(B, 4, T, H, W, device=dev, generator=g) * 0.18215 * 5.0,
                 "context": torch.randn(B, 77, 1024, device=dev, generator=g).to(BF),
                 "image_tokens": torch.randn(B, 257, 1280, device=dev, generator=g).to(BF),
                 "fps": torch.randint(1, 30, (B,), device=dev, generator=g), "null_context": null_ctx, "null_image_tokens": null_tok}
        loss = flow.training_step(batch)
        loss.backward()
        opt.step()
        losses.append(loss.detach().reshape(1))

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    opt.check_errors()
    lv = [float(v) for v in torch.cat(losses).cpu()]
    nu = sum(p.numel() for p in flow.model.parameters()) / 1e9
    nr = sum(p.numel() for p in flow.image_proj_model.parameters()) / 1e6
    res = {"metric": "finetune samples/sec, DynamiCrafter I2V (Resampler + UNet) full-FT bf16", "value": B * steps / el, "unit": "samples/s", "n_gpus": 1,
           "steps": steps, "warmup": warmup, "ms_per_step": 1000.0 * el / steps, "higher_is_better": True, "dtype": "bf16", "data": "synthetic",
           "config": {"workload": f"LatentVisualDiffusionFlow.training_step (configs/002_dynamicrafter): latents [{B},4,16,{H},{W}] (+ 4 conditioning-frame "
                                  f"channels), text context [{B},77,1024], image tokens [{B},257,1280] -> Resampler -> 16 tokens per frame, fps random; v target, "
                                  f"use_scale, zero-terminal-SNR schedule, three-way condition dropout (p 0.05), random conditioning frame; {nu:.2f} B UNet + "
                                  f"{nr:.1f} M Resampler weights trained (fp32 masters + fused AdamW), no activation recompute, train mode: ResBlock + "
                                  "TemporalConvBlock dropout 0.1",
                      "micro_batch": B, "latents": "pre-encoded (synthetic)", "text / image tokens": "pre-encoded OpenCLIP outputs (synthetic)"},
           "peak_hbm_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 1), "loss_first": lv[0], "loss_last": lv[-1]}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernel,step40,step72")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=500, help="seconds per child process")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child is not None:
        if args.child == "kernel":
            bench_kernel(args.rounds, args.iters)
        elif args.child in ("step40", "step72"):
            bench_step((40, 64) if args.child == "step40" else (72, 128), 4 if args.child == "step40" else 2, args.steps, args.warmup)
        else:
            raise SystemExit(f"unknown part {args.child!r}")
        return 0
    for part in args.parts.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", part, "--rounds", str(args.rounds), "--iters", str(args.iters),
               "--steps", str(args.steps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, timeout=args.timeout)
        if r.returncode != 0:             # a child that fails ends the run: nothing more is started on the device
            print(json.dumps({"part": part, "error": f"child exited with {r.returncode}"}), flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
