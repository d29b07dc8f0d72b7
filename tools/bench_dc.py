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
  clip     gradient clipping's kernels alone on a 1.41 B-element fp32 buffer (the UNet's flat gradient) and on a 1.8 M-element one (CogVideoX
           LoRA): the norm pass + finalise (vt_grad_sqnorm + vt_clip_finalize, 4 bytes per element read), the vt_adamw launch and the
           vt_adamw_clip launch (30 bytes per element moved) -- HIP events, ms per launch, the three alternate inside every round; medians
           and spreads as the kernel part reports them, and the norm pass as a fraction of the vt_adamw launch of the same run.
  step40_ab  the step40 workload with and without gradient clipping (--clip, default 0.5 here) in ONE process: one flow, two joint
           optimizers on its training state (their moments are separate), blocks of --steps steps alternating off / on for --rounds rounds.
``--clip VAL`` runs step40 / step72 with gradient_clip_val VAL (default: off, so earlier lines stay comparable).
The step parts each run in a child process (a fresh allocator, its own time limit).

    python tools/bench_dc.py [--parts kernel,step40,step72,clip,step40_ab] [--rounds 5] [--steps 4] [--warmup 2] [--timeout 500] [--clip VAL]
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


def bench_clip(rounds: int, iters: int):
    sys.path.insert(0, ROOT)
    import torch
    from vt355 import ops
    dev = torch.device("cuda:0")
    P = ops.grad_sqnorm_partials()
    out = {"metric": "gradient clipping kernels alone: norm pass + finalise, vt_adamw, vt_adamw_clip", "unit": "ms per launch", "rounds": rounds,
           "iters_per_round": iters, "norm_pass_grid": [P, 256], "sizes": []}
    for n in (1_410_000_000, 1_800_000):
        g = torch.Generator(device=dev).manual_seed(n % 1000)
        p = torch.randn(n, device=dev, generator=g)
        gr = torch.randn(n, device=dev, generator=g).mul_(1e-3)
        m, v, pb = torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.empty(n, dtype=torch.bfloat16, device=dev)
        partials, record = torch.empty(P, device=dev), torch.zeros(2, device=dev)
        step = {"n": 0}

        def norm():
            ops.grad_sqnorm(gr, partials, 0)
            ops.clip_finalize(partials, 1, 1.0, 0.5, record)

        def adamw(**kw):
            step["n"] += 1
            ops.adamw(p, gr, m, v, pb, 1e-5, 0.9, 0.999, 1e-8, 1e-2, step["n"], 1.0, None, **kw)

        coef = record[1:2]
        fns = {"norm_pass": norm, "adamw": adamw, "adamw_clip": lambda: adamw(clip_coef=coef)}

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / iters

        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                times[k].append(timed(fn))
        sz = {"elements": n, "total_norm": float(record[0]), "clip_coef": float(record[1])}
        for k, t in times.items():
            med = statistics.median(t)
            sz[k] = {"median_ms": round(med, 4), "spread_ms": round(max(t) - min(t), 4),
                     "gbps": round((4.0 if k == "norm_pass" else 30.0) * n / 1e9 / (med / 1e3), 1)}
        sz["norm_pass_over_adamw"] = round(sz["norm_pass"]["median_ms"] / sz["adamw"]["median_ms"], 4)
        a, c = sz["adamw"], sz["adamw_clip"]
        sz["adamw_clip_minus_adamw_ms"] = round(c["median_ms"] - a["median_ms"], 4)
        sz["adamw_clip_separable_beyond_spread"] = bool(abs(c["median_ms"] - a["median_ms"]) > max(a["spread_ms"], c["spread_ms"]))
        out["sizes"].append(sz)
        del p, gr, m, v, pb
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


def bench_step(latent_hw, B: int, steps: int, warmup: int, clip: float = 0.0, ab_rounds: int = 0):
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
    opts = {"off": flow.configure_optimizers()} if (ab_rounds or not clip > 0.0) else {}
    if clip > 0.0:
        opts["clip"] = flow.configure_optimizers(gradient_clip_val=clip)
    opt = next(iter(opts.values()))
    g = torch.Generator(device=dev).manual_seed(20230211)
    null_ctx = torch.randn(77, 1024, device=dev, generator=g).to(BF)            # stand for the encodings of "" and of an all-zero image
    null_tok = torch.randn(257, 1280, device=dev, generator=g).to(BF)
    losses, opt_events = [], {}

    def step(opt=opt):
        opt.zero_grad()
        batch = {"latents": torch.randn(B, 4, T, H, W, device=dev, generator=g) * 0.18215 * 5.0,
                 "context": torch.randn(B, 77, 1024, device=dev, generator=g).to(BF),
                 "image_tokens": torch.randn(B, 257, 1280, device=dev, generator=g).to(BF),
                 "fps": torch.randint(1, 30, (B,), device=dev, generator=g), "null_context": null_ctx, "null_image_tokens": null_tok}
        loss = flow.training_step(batch)
        loss.backward()
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        h0 = time.perf_counter()
        opt.step()
        host = 1000.0 * (time.perf_counter() - h0)
        ev[1].record()
        opt_events.setdefault(id(opt), []).append(ev + (host,))
        losses.append(loss.detach().reshape(1))

    if ab_rounds:
        for o in opts.values():
            for _ in range(warmup):
                step(o)
        times = {k: [] for k in opts}
        opt_events.clear()
        # Pauses of Python's cyclic collector: the step synchronises with the host (condition dropout, dropout seeds), so a pause is device
        # idle time, and their period (several steps) can alias with the alternation.  Counted per variant so that they are not read as the option's.
        import gc
        pauses, cur = {k: [] for k in opts}, {"k": None, "t": 0.0}

        def on_gc(phase, info):
            if phase == "start":
                cur["t"] = time.perf_counter()
            elif cur["k"] is not None and info["generation"] == 2:
                pauses[cur["k"]].append(round(1000.0 * (time.perf_counter() - cur["t"]), 1))

        gc.callbacks.append(on_gc)
        for _ in range(ab_rounds):
            for k, o in opts.items():
                cur["k"] = k
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    step(o)
                torch.cuda.synchronize()
                times[k].append(1000.0 * (time.perf_counter() - t0) / steps)
        gc.callbacks.remove(on_gc)
        for o in opts.values():
            o.check_errors()
        res = {"metric": "DynamiCrafter I2V full-FT step with and without gradient clipping, same process, alternating", "unit": "ms per step",
               "latents": [B, 4, T, H, W], "gradient_clip_val": clip, "rounds": ab_rounds, "steps_per_block": steps, "warmup_per_optimizer": warmup,
               "grad_norm_last": float(opts["clip"].grad_norm), "loss_last": float(losses[-1])}
        for k, t in times.items():
            res[k] = {"median_ms": round(statistics.median(t), 3), "spread_ms": round(max(t) - min(t), 3), "rounds_ms": [round(x, 3) for x in t],
                      # device time between the events around optimizer.step(): the norm passes, the finalise and the AdamW launches
                      "optimizer_device_ms_median": round(statistics.median(a.elapsed_time(b) for a, b, _ in opt_events[id(opts[k])]), 3),
                      "optimizer_device_ms_max": round(max(a.elapsed_time(b) for a, b, _ in opt_events[id(opts[k])]), 3),
                      "optimizer_host_ms_median": round(statistics.median(h for _, _, h in opt_events[id(opts[k])]), 3),
                      # device time from the end of one optimizer step to the end of the next, steps 2.. of every block
                      "step_device_ms": [round(e[i][1].elapsed_time(e[i + 1][1]), 1) for e in [opt_events[id(opts[k])]]
                                         for i in range(len(e) - 1) if (i + 1) % steps],
                      "host_gc_gen2_pauses_ms": pauses[k]}
            res[k]["step_device_ms_median"] = statistics.median(res[k]["step_device_ms"])
        res["clip_minus_off_ms"] = round(res["clip"]["median_ms"] - res["off"]["median_ms"], 3)
        res["inside_spread"] = bool(abs(res["clip_minus_off_ms"]) <= max(res["clip"]["spread_ms"], res["off"]["spread_ms"]))
        res["clip_minus_off_step_device_median_ms"] = round(res["clip"]["step_device_ms_median"] - res["off"]["step_device_ms_median"], 2)
        print(json.dumps(res), flush=True)
        return
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
                      "micro_batch": B, "gradient_clip_val": clip if clip > 0.0 else None, "latents": "pre-encoded (synthetic)", "text / image tokens": "pre-encoded OpenCLIP outputs (synthetic)"},
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
    ap.add_argument("--clip", type=float, default=None, help="gradient_clip_val of the step parts (default: off; step40_ab: 0.5)")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child is not None:
        if args.child == "kernel":
            bench_kernel(args.rounds, args.iters)
        elif args.child == "clip":
            bench_clip(args.rounds, args.iters)
        elif args.child == "step40_ab":
            bench_step((40, 64), 4, args.steps, args.warmup, 0.5 if args.clip is None else args.clip, ab_rounds=args.rounds)
        elif args.child in ("step40", "step72"):
            bench_step((40, 64) if args.child == "step40" else (72, 128), 4 if args.child == "step40" else 2, args.steps, args.warmup,
                       args.clip or 0.0)
        else:
            raise SystemExit(f"unknown part {args.child!r}")
        return 0
    for part in args.parts.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", part, "--rounds", str(args.rounds), "--iters", str(args.iters),
               "--steps", str(args.steps), "--warmup", str(args.warmup)] + ([] if args.clip is None else ["--clip", str(args.clip)])
        r = subprocess.run(cmd, timeout=args.timeout)
        if r.returncode != 0:             # a child that fails ends the run: nothing more is started on the device
            print(json.dumps({"part": part, "error": f"child exited with {r.returncode}"}), flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
