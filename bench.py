#!/usr/bin/env python3
"""bench.py -- finetune samples/sec + step time, CogVideoX-2B T2V LoRA 49x480x720 bf16 (BASELINE.json metric).

One "step" = one optimizer step of the reference recipe (configs/004_cogvideox/cogvideo2b.yaml: batch_size 2,
accumulate_grad_batches 2 = 4 samples per optimizer step and rank).  LoRA default: the four samples run as ONE batch (--micro-batch 4
--accum 1: the same gradient as 2 x 2, 122 of the 288 GB; pass --micro-batch 2 --accum 2 for the YAML's literal schedule, which the full
fine-tune default keeps): synthetic latents [B,13,16,60,90] + text [B,226,4096]
already resident in HBM -> add_noise -> DiT forward -> loss -> backward (LoRA grads) -> [DDP all-reduce] -> fused AdamW.
Random-init weights of the 2B architecture (no checkpoints offline), nothing skipped inside the timed region.

A plain run sets up, warms up, times --steps optimizer steps and prints one JSON line (metric, value, unit, higher_is_better, dtype,
ms_per_step = wall milliseconds of one timed step).  --full adds what takes extra work: HIP-event times of the attention / GEMM /
convolution launches inside the timed steps (`kernels`, `roofline`, `roofline_more`), the CPU-oracle baseline (`cpu_baseline`) and,
for --model hunyuan --fp8, the same batch's loss in bf16.  --dump-outputs DIR writes, after the timed steps, what the last timed
step computed (loss, the denoiser's prediction, the trained parameters after the update and their gradients) as float32 .npy files.

  python bench.py --gpus 1 --steps 5 --warmup 2
  python bench.py --gpus 1 --steps 5 --warmup 2 --full                  # + per-kernel times, roofline, CPU baseline
  python bench.py --gpus 1 --steps 5 --warmup 2 --dump-outputs DIR      # + the last timed step's outputs as DIR/*.npy
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def launch_ranks(n: int, argv) -> int:
    """`python bench.py --gpus N` without a launcher around it: start the N ranks ourselves, one process per GPU as PL's
    DDPStrategy does (videotuna/utils/train_utils.py:127-139, scripts/train.py:215-217).  Runs BEFORE this process
    imports torch or touches the GPU (children are fresh interpreters, nothing is exec'ed over a process that holds a
    device); rank 0's stdout is this process's stdout, so its JSON line is the output.  Non-zero when any rank fails;
    the remaining ranks are then terminated by PID."""
    import signal
    import socket
    import subprocess
    why = _gpu_runtime_preloaded()
    if why:
        # a profiler (rocprofv3 --pmc ...) or any HIP preload initialises the GPU in THIS process before main() runs: starting the ranks
        # from here would be a fork + exec out of a process that holds a device.  Profile per rank instead: `--gpus 1`, or ranks started
        # by an external launcher (torch.distributed.run) before anything touches the GPU.
        print(f"bench.py: refusing to self-launch {n} ranks: {why}. Profile one rank (`--gpus 1`), or start the ranks with "
              f"`python -m torch.distributed.run --nproc-per-node {n} bench.py --gpus {n} ...` outside the profiler.", file=sys.stderr, flush=True)
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []

    def _stop(signum, _frame):            # an interrupted launcher must not leave ranks holding the GPUs
        for pr in procs:
            if pr.poll() is None:
                pr.terminate()
        deadline = time.time() + 10
        for pr in procs:
            try:
                pr.wait(max(0.1, deadline - time.time()))
            except subprocess.TimeoutExpired:
                pr.kill()
        sys.exit(128 + signum)
    for sg in (signal.SIGINT, signal.SIGTERM):
        signal.signal(sg, _stop)
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc, live = 0, set(range(n))
    while live:
        for r in sorted(live):
            code = procs[r].poll()
            if code is None:
                continue
            live.discard(r)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 1
                print(f"bench.py: rank {r} exited with code {code}; stopping the other ranks", file=sys.stderr, flush=True)
                for o in live:
                    procs[o].terminate()
        time.sleep(0.05)
    return rc


def _gpu_runtime_preloaded() -> str:
    """non-empty when something has (or will have) initialised HIP in this process before our code ran: a profiler's tool library or any
    LD_PRELOAD, or the HIP runtime / rocprofiler-sdk already mapped"""
    if os.environ.get("LD_PRELOAD"):
        return f"LD_PRELOAD={os.environ['LD_PRELOAD']!r} is set"
    for k in os.environ:
        if k.startswith(("ROCPROFILER", "ROCP_", "ROCPROF_")) or k in ("HSA_TOOLS_LIB", "ROCTRACER_DOMAIN"):
            return f"profiler environment variable {k} is set"
    try:
        with open("/proc/self/maps") as f:
            maps = f.read()
        for lib in ("libamdhip64", "librocprofiler-sdk", "libhsa-runtime64"):
            if lib in maps:
                return f"{lib} is already mapped into the launcher process"
    except OSError:
        pass
    return ""


def _wants_launch(argv):
    """--gpus N > 1 with no rendezvous environment around us -> we are the launcher"""
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--gpus", type=int, default=1)
    n = ap.parse_known_args(argv)[0].gpus
    return n if (n > 1 and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ) else 0


if __name__ == "__main__" and _wants_launch(sys.argv[1:]):
    sys.exit(launch_ranks(_wants_launch(sys.argv[1:]), sys.argv[1:]))

import torch
import torch.distributed as dist

DUMP_CAP = 5_000_000        # elements per dumped array (20 MB of float32); a larger array is written as a fixed, seeded sample
DUMP_LIMIT = 64_000_000     # bytes of all dumped arrays together (64 MB)


def dump_outputs(path, arrays):
    """--dump-outputs: name -> tensor, written as path/<name>.npy in float32.  An array of more than DUMP_CAP elements is replaced by
    DUMP_CAP of its (flattened) elements at sorted indices drawn from a fixed seed, so two runs of the same arguments sample the same
    elements.  Returns name -> {"shape", "sampled"} for the result line."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    out, total = {}, 0
    for name, t in arrays.items():
        t = t.detach()
        flat = t.reshape(-1)
        sampled = flat.numel() > DUMP_CAP
        if sampled:
            idx = torch.randint(0, flat.numel(), (DUMP_CAP,), generator=torch.Generator().manual_seed(0)).sort().values
            flat = flat[idx.to(flat.device)]
        a = flat.to(torch.float32).cpu().numpy()
        if not sampled:
            a = a.reshape(tuple(t.shape))
        total += a.nbytes
        assert total <= DUMP_LIMIT, f"--dump-outputs: more than {DUMP_LIMIT} bytes"
        np.save(os.path.join(path, name + ".npy"), a)
        out[name] = {"shape": list(t.shape), "sampled": DUMP_CAP if sampled else None}
    return out


def cpu_baseline(seconds_budget=40.0):
    """The oracle (CPU restatement of the reference path) timed on the host cores: ONE full-size CogVideoX-2B block,
    forward + backward, B=1, S=17776, fp32 eager; a sample needs 30 such blocks (embeddings/final < 0.1 % of FLOPs)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import cogvideox_oracle as O
    cfg = O.DiTConfig(num_layers=1)
    torch.manual_seed(0)
    P = {k: v for k, v in O.init_params(cfg, 0).items() if k.startswith("transformer_blocks.0.")}
    Lo = O.init_lora(cfg, r=4, seed=1, zero_b=False)
    for v in Lo.values():
        v.requires_grad_(True)
    St, Sv, d = 226, 17550, cfg.inner_dim
    h_txt = torch.randn(1, St, d); h_vid = torch.randn(1, Sv, d).requires_grad_(True)   # dX must flow to earlier blocks
    emb = torch.randn(1, cfg.time_embed_dim)
    t0 = time.time()
    ht, hv = O.dit_block(h_txt, h_vid, emb, P, "transformer_blocks.0.", cfg, Lo, 0.25)
    (hv.sum() + ht.sum()).backward()
    dt = time.time() - t0
    threads = torch.get_num_threads()
    cpu_model = ""
    try:
        with open("/proc/cpuinfo") as f:
            cpu_model = [l.split(":", 1)[1].strip() for l in f if l.startswith("model name")][0]
    except Exception:
        pass
    return {"value": 1.0 / (30.0 * dt), "unit": "samples/s", "cores": threads, "kind": "port", "cpu_model": cpu_model,
            "sample": f"1 of 30 DiT blocks, fwd+bwd, B=1, S=17776, fp32 eager PyTorch-CPU oracle, {dt:.1f} s measured, x30",
            "block_seconds": dt, "host_cpus": os.cpu_count()}


def bench_vc2(args):
    """BASELINE configs[3]: VideoCrafter2 T2V 320x512 UNet (configs/001_videocrafter2/vc2_t2v_320x512.yaml: batch_size 4, 16 frames,
    latents [4,4,16,40,64], context [4,77,1024], fps 24), full fine-tune: q_sample -> UNet -> eps-MSE -> backward -> fused AdamW.
    One step = one optimizer step on one micro-batch of 4 samples (--accum 1 default here; the yaml's trainer accumulates 2)."""
    from vt355 import ops
    from vt355.ddp import FlatGradReducer, broadcast_flat, init_from_env
    from vt355.lvdm import LVDMFlow
    rank, local, world = init_from_env(os.environ.get("VT_DDP_BACKEND"))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    if os.environ.get("VT_ONE_GPU") == "1":
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    unet = dict(target="vt355.unet.UNetModel", params=dict(
        in_channels=4, out_channels=4, model_channels=320, attention_resolutions=[4, 2, 1], num_res_blocks=2, channel_mult=[1, 2, 4, 4],
        num_head_channels=64, transformer_depth=1, context_dim=1024, use_linear=True, use_checkpoint=True, temporal_conv=True,
        temporal_attention=True, temporal_selfatt_only=True, use_relative_position=False, use_causal_attention=False,
        temporal_length=16, addition_attention=True, fps_cond=True))
    lora = args.mode == "lora" and getattr(args, "mode_given", False)          # --model vc2 --mode lora: configs/001_videocrafter2/vc2_t2v_lora.yaml
    flow = LVDMFlow(denoiser_config=unet, scheduler_config=dict(target="vt355.lvdm.LDDPM", params=dict(timesteps=1000, linear_start=0.00085, linear_end=0.012)),
                    use_scale=True, scale_b=0.7, base_learning_rate=6e-6,
                    lora_args=({"target_modules": ["to_q", "to_k", "to_v"], "lora_rank": 4, "lora_alpha": 1, "lora_dropout": 0.0} if lora else None))
    flow.unet.init_weights(1234) if lora else flow.model.init_weights(1234)
    flow.to(dev)
    if lora:
        flow.inject_lora()                       # scripts/train.py:168-169
        flow.unet.lora.init_weights(5, zero_b=False)
    opt = flow.configure_optimizers()
    ts = flow.unet.lora.train_state if lora else flow.model.train_state
    broadcast_flat(ts.flat); broadcast_flat(ts.flat_bf16)
    red = FlatGradReducer(ts.grad)
    B = args.micro_batch if args.micro_batch is not None else 4   # the recipe's batch_size
    accum = args.accum if args.accum is not None else 1
    dgen = torch.Generator(device=dev).manual_seed(20230211 + rank)
    null_ctx = torch.randn(77, 1024, device=dev, generator=dgen).to(torch.bfloat16)      # stands for the OpenCLIP embedding of the empty prompt

    def make_batch():
        z = torch.randn(B, 4, 16, 40, 64, device=dev, generator=dgen) * 0.18215 * 5.0
        ctx = (torch.randn(B, 77, 1024, device=dev, generator=dgen)).to(torch.bfloat16)
        noise = torch.randn(B, 4, 16, 40, 64, device=dev, generator=dgen)
        t = torch.randint(0, 1000, (B,), device=dev, generator=dgen)
        ctx = flow.random_uncond(ctx, null_ctx)            # classifier-free-guidance dropout of the caption, uncond_prob 0.2 (ddpm3d.py:710-722)
        return z, ctx, noise, t

    losses = []

    def step():
        opt.zero_grad()
        for _ in range(accum):
            z, ctx, noise, t = make_batch()
            loss = flow.loss_from(z, ctx, t, noise, fps=24)
            (loss / accum).backward()
            losses.append(loss.detach())
        red.reduce_async(); red.wait()
        opt.step(grad_scale=red.grad_scale)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    ops.profile_reset(args.full)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    elapsed = time.perf_counter() - t0
    prof, work = ops.profile_collect(), ops.profile_work()
    ops.profile_reset(False)
    opt.check_errors()
    if world > 1:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = tt.item()
    samples = world * B * accum * args.steps
    if rank == 0:
        lv = [float(x) for x in torch.stack(losses[-accum * args.steps:]).cpu()]
        kern = {}
        for name, (ms, n) in prof.items():
            kern[name] = {"avg_ms": ms, "launches": n}
            if name in work:
                kern[name]["tflops_algorithmic"] = work[name] / (ms * n) / 1e9
        fwd_tflop = 12.58            # measured with FlopCounterMode on the imported reference UNet, per sample
        step_tflop = 3.0 * fwd_tflop * B * accum
        ach = kern.get("conv", {}).get("tflops_algorithmic")
        res = {"metric": "finetune samples/sec, VideoCrafter2 T2V 320x512 UNet %s bf16" % ("LoRA r=4" if lora else "full-FT"), "value": samples / elapsed, "unit": "samples/s",
               "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1000.0 * elapsed / args.steps,
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
               "config": {"workload": "VideoCrafter2 T2V 320x512 UNet (configs[3], NOT the headline config): latents [4,4,16,40,64], context "
                                      "[4,77,1024], fps 24, " + ("base weights frozen, rank-4 adapters on to_q / to_k / to_v of every CrossAttention trained (vc2_t2v_lora.yaml), "
                                                                 if lora else "all 1.41 B weights trained (fp32 master + fused AdamW), ") + "no activation recompute, train mode: "
                                      "TemporalConvBlock dropout 0.1 and caption dropout (uncond_prob 0.2) on, as the reference trains",
                          "micro_batch": B, "accumulate_grad_batches": accum, "global_batch": world * B * accum, "parallelism": f"dp{world}",
                          "weights": "seeded random init (no checkpoints offline)", "latents": "pre-encoded latents (synthetic)",
                          "text": "pre-encoded OpenCLIP embeddings (synthetic)"},
               "peak_hbm_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 1),
               "step_tflops_algorithmic": step_tflop * args.steps / elapsed, "loss_first": lv[0], "loss_last": lv[-1]}
        if args.full:
            res["roofline"] = {"bound": "mfma", "kernel": "convnd_cl_kernel / convnd320_kernel", "achieved": ach, "peak": 2500.0, "unit": "TFLOP/s",
                               "frac": (ach / 2500.0) if ach else None, "traffic": None,
                               "note": "all forward / input-gradient convolutions of the step, 2*M*Cout*taps*Cin FLOPs each, HIP events on the launch stream"}
            res["kernels"] = kern
        print(json.dumps(res), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def bench_stdit(args):
    """BASELINE configs[0] at its stated size on the GPU (the config itself is a CPU-eager plumbing step in the reference): OpenSora v1.0
    STDiT-XL/2, latents [B,4,16,32,32] (16x256x256 video), T5 embeddings [B,1,120,4096] with ragged masks, full fine-tune of 759.6 M
    weights: q_sample -> STDiT -> mse + VB loss -> backward -> fused AdamW."""
    from vt355 import ops
    from vt355.ddp import init_from_env
    from vt355.stdit import OpenSoraFlow
    rank, local, world = init_from_env(os.environ.get("VT_DDP_BACKEND"))
    assert world == args.gpus == 1, "the OpenSora line is single-GPU"
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    flow = OpenSoraFlow(unet_config=dict(target="vt355.stdit.STDiT_XL_2", params=dict(space_scale=0.5, time_scale=1.0, input_size=[16, 32, 32],
                                                                                      class_dropout_prob=0.0)),
                        diffusion_scheduler_config=dict(target="vt355.stdit.OpenSoraScheduler", params=dict(timesteps=1000)),
                        base_learning_rate=6e-6, use_scale=True, scale_b=0.7)
    flow.model.init_weights(7)
    flow.to(dev)
    opt = flow.configure_optimizers()
    B = args.micro_batch if args.micro_batch is not None else 4   # the yaml's batch_size
    dgen = torch.Generator(device=dev).manual_seed(20230211)
    mask = torch.zeros(B, 120, dtype=torch.int64, device=dev)
    for b in range(B):
        mask[b, :20 + 25 * b] = 1
    losses = []

    def step():
        opt.zero_grad()
        z = torch.randn(B, 4, 16, 32, 32, device=dev, generator=dgen)
        y = torch.randn(B, 1, 120, 4096, device=dev, generator=dgen).to(torch.bfloat16)
        t = torch.randint(0, 1000, (B,), device=dev, generator=dgen)
        z = z * flow.scale_arr[t].view(-1, 1, 1, 1, 1)
        loss = flow.loss_from(z, y, mask, t, torch.randn(z.shape, device=dev, generator=dgen))
        loss.backward()
        losses.append(loss.detach())
        opt.step()

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    lv = [float(x) for x in torch.stack(losses[-args.steps:]).cpu()]
    fwd_tflop = 5.64             # FlopCounterMode on the imported reference STDiT-XL/2, per sample
    print(json.dumps({"metric": "finetune samples/sec, OpenSora-v1.0 STDiT-XL/2 16x256x256 full-FT bf16", "value": B * args.steps / elapsed,
                      "unit": "samples/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1000.0 * elapsed / args.steps,
                      "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
                      "config": {"workload": "OpenSora v1.0 STDiT-XL/2 (configs[0] at its stated size, NOT the headline config): latents "
                                             f"[{B},4,16,32,32], T5 embeddings [{B},1,120,4096] with ragged masks, all 759.6 M weights trained",
                                 "micro_batch": B, "weights": "seeded random init (no checkpoints offline)"},
                      "peak_hbm_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 1),
                      "step_tflops_algorithmic": 3.0 * fwd_tflop * B * args.steps / elapsed, "loss_first": lv[0], "loss_last": lv[-1]}), flush=True)


def bench_hunyuan(args):
    """extra data point: the HunyuanVideo block trunk (vt355.hunyuan.HunyuanBlocks) at the shipped recipe's sequence -- 544x960x17f =
    10 200 image tokens + 256 text tokens (ragged), d = 3072, 24 x 128 -- at a REDUCED DEPTH (4 double + 8 single of the model's 20 + 40:
    the full 12.8 B-parameter trunk does not fit one GPU with fp32 master weights and Adam moments), full fine-tune of those blocks,
    flow-matching loss on the image rows."""
    import torch
    from vt355 import ops
    from vt355.ddp import init_from_env
    from vt355.hunyuan import HunyuanBlocks, flow_matching_loss
    from vt355.optim import FusedAdamW
    import torch.distributed as dist
    from vt355.ddp import FlatGradReducer
    rank, local, world = init_from_env(os.environ.get("VT_DDP_BACKEND"))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    if os.environ.get("VT_ONE_GPU") == "1":
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    lora = args.mode == "lora" and os.environ.get("VT_HY_FULLFT") is None
    if lora:
        # the whole trunk: frozen block weights (25.7 GB bf16) + rank-4 adapters, as the shipped recipe trains (--layers: debug depth)
        nd, ns = (20, 40) if args.layers == 30 else (max(1, args.layers // 3), max(1, args.layers - args.layers // 3))
    else:
        assert world == 1, "the full-FT block-trunk line is single-GPU"
        nd, ns = (4, 8) if args.layers == 30 else (max(1, args.layers // 3), max(1, args.layers - args.layers // 3))
    lT, lH, lW = (int(v) for v in args.latent.split(","))
    D, H, Li, Lt = 3072, 24, lT * (lH // 2) * (lW // 2), 256
    sp_deg = args.sp
    assert world % sp_deg == 0 and H % sp_deg == 0 and Li % sp_deg == 0, (world, sp_deg, Li)
    n_dp, dp_idx = world // sp_deg, rank // sp_deg
    B = args.micro_batch if args.micro_batch is not None else 1
    g = torch.Generator(device=dev).manual_seed(20230211 + dp_idx)          # the ranks of a sequence-parallel group see the same batch
    tv = torch.tensor([Lt - 37 * (b % 5) for b in range(B)], device=dev)
    losses = []
    ops.profile_reset(args.full)
    if lora:
        # the WHOLE denoiser (patch embed, token refiner, modulation vector, 20 + 40 blocks, final layer) through the workflow's training_step:
        # latents [B, 16, T, H, W] (default 5 x 68 x 120 = 544x960x17f after the 4x8x8 VAE -> 10 200 tokens; 33,90,160 = 720p x 129f -> 118 800),
        # LLM embeddings [B, 256, 4096] (ragged), CLIP pooled [B, 768]
        from vt355.hunyuan import HYVideoDiffusionTransformer, HunyuanVideoFlow
        model = HYVideoDiffusionTransformer(mm_double_blocks_depth=nd, mm_single_blocks_depth=ns, lora_rank=4, fp8=bool(args.fp8)).to(dev).init_weights(11)
        model.lora.init_weights(12, zero_b=False)
        if sp_deg > 1:        # every rank creates every group; image tokens of a sample split over the sp_deg ranks of its group (vt355.sp)
            groups = [dist.new_group(list(range(i * sp_deg, (i + 1) * sp_deg))) for i in range(n_dp)]
            model.set_sequence_parallel(groups[dp_idx])
            torch.manual_seed(977 + rank)      # training_step's own draws (sigma, noise): not the batch generator's stream
        flow = HunyuanVideoFlow(model=model, learning_rate=1e-5).to(dev)
        opt = flow.configure_optimizers()
        red = FlatGradReducer(model.lora.train_state.grad)                  # adapters: ONE all-reduce over all ranks (data and sequence parallel alike)
        mask = (torch.arange(Lt, device=dev)[None, :] < tv[:, None]).long()

        def make_batch(gen):
            return {"latents": torch.randn(B, 16, lT, lH, lW, device=dev, generator=gen),
                    "prompt_embeds": torch.randn(B, Lt, 4096, device=dev, generator=gen).to(torch.bfloat16), "prompt_attention_mask": mask,
                    "pooled_prompt_embeds": torch.randn(B, 768, device=dev, generator=gen).to(torch.bfloat16)}

        def loss_only():          # one fixed batch, fixed sigma / noise draws: the fp8-vs-bf16 loss comparison of the --fp8 line
            torch.manual_seed(4242)
            with torch.no_grad():
                return float(flow.training_step(make_batch(torch.Generator(device=dev).manual_seed(99))))

        def step():
            batch = make_batch(g)
            loss = flow.training_step(batch)
            loss.backward()
            losses.append(loss.detach())
            red.reduce()
            opt.step(grad_scale=red.grad_scale)
    else:
        model = HunyuanBlocks(hidden_size=D, heads_num=H, mm_double_blocks_depth=nd, mm_single_blocks_depth=ns, fp8=bool(args.fp8)).to(dev).init_weights(11)
        ts = model.enable_training()
        opt = FusedAdamW(ts.params, lr=1e-5, fullft_state=ts)
        ang = torch.rand(Li, 64, device=dev, generator=g) * 6.28
        freqs = (torch.repeat_interleave(ang.cos(), 2, dim=1).contiguous(), torch.repeat_interleave(ang.sin(), 2, dim=1).contiguous())

        def loss_only():
            gg = torch.Generator(device=dev).manual_seed(99)
            with torch.no_grad():
                out = model(torch.randn(B, Li, D, device=dev, generator=gg).to(torch.bfloat16), torch.randn(B, Lt, D, device=dev, generator=gg).to(torch.bfloat16),
                            torch.randn(B, D, device=dev, generator=gg).to(torch.bfloat16), tv, freqs)
                return float(flow_matching_loss(out[:, :Li].contiguous(), torch.randn(B, Li, D, device=dev, generator=gg), torch.randn(B, Li, D, device=dev, generator=gg))[0])

        def step():
            img = torch.randn(B, Li, D, device=dev, generator=g).to(torch.bfloat16)
            txt = torch.randn(B, Lt, D, device=dev, generator=g).to(torch.bfloat16)
            vec = torch.randn(B, D, device=dev, generator=g).to(torch.bfloat16)
            x0 = torch.randn(B, Li, D, device=dev, generator=g); noise = torch.randn(B, Li, D, device=dev, generator=g)
            out = model(img, txt, vec, tv, freqs)
            loss, dpred = flow_matching_loss(out[:, :Li].contiguous(), x0, noise)
            dfull = torch.zeros_like(out); dfull[:, :Li] = dpred
            out.backward(dfull)
            losses.append(loss.detach())
            opt.step()

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    fp8_cmp = None
    if args.fp8 and world == 1 and args.full:      # the same batch through the E4M3 weights and through the bf16 weights they were rounded from
        def repack(mode):
            model.fp8 = mode; model._packed = None
            if model.lora is not None:
                model.lora._packed = None
        l8 = loss_only(); repack(False); lb = loss_only(); repack(True)
        fp8_cmp = {"loss_fp8": l8, "loss_bf16": lb, "rel_delta": abs(l8 - lb) / max(abs(lb), 1e-30)}
    for _ in range(args.warmup):
        step()
    barrier()
    ops.profile_reset(args.full)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    elapsed = time.perf_counter() - t0
    prof, work = ops.profile_collect(), ops.profile_work()
    ops.profile_reset(False)
    if world > 1:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = tt.item()
    if rank != 0:
        if world > 1:
            dist.barrier(); dist.destroy_process_group()
        return
    kern = {k: {"avg_ms": ms, "launches": n, **({"tflops_algorithmic": work[k] / (ms * n) / 1e9} if work.get(k) else {})} for k, (ms, n) in prof.items()}
    S = Li + Lt
    # per block forward: linears + attention 4 S^2 d; double: img+txt streams (qkv, proj, fc1, fc2 = 24 S d^2 over both streams); single: linear1 + linear2
    fwd_double = 24.0 * S * D * D + 4.0 * S * S * D
    fwd_single = 2.0 * S * D * (3 * D + 4 * D) + 2.0 * S * (D + 4 * D) * D + 4.0 * S * S * D
    att = 4.0 * S * S * D
    if lora:    # forward + backward without the frozen weights' dW: linears 2x, attention 3x
        step_tf = B * n_dp * (nd * (2.0 * (fwd_double - att) + 3.0 * att) + ns * (2.0 * (fwd_single - att) + 3.0 * att)) / 1e12
    else:
        step_tf = 3.0 * B * (nd * fwd_double + ns * fwd_single) / 1e12
    lv = [float(x) for x in torch.stack(losses[-args.steps:]).cpu()]
    size = f"latents 16x{lT}x{lH}x{lW}"
    print(json.dumps({"metric": (f"finetune samples/sec, HunyuanVideo-T2V denoiser (whole HYVideoDiffusionTransformer, {nd} + {ns} blocks) {size} LoRA r=4 bf16" if lora else
                                 "finetune samples/sec, HunyuanVideo block trunk (%d double + %d single of 20 + 40) 544x960x17f full-FT bf16" % (nd, ns)),
                      "value": B * n_dp * args.steps / elapsed, "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                      "ms_per_step": 1000.0 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
                      "data": "synthetic",
                      "config": {"workload": ("HunyuanVideo-T2V denoiser through HunyuanVideoFlow.training_step (configs[4] family, " + size + ", "
                                              "NOT the headline config): patch embed + token refiner + " if lora else
                                              "HunyuanVideo MMDoubleStreamBlock / MMSingleStreamBlock trunk (configs[4] family, NOT the headline config and "
                                              "NOT the whole model): ") + f"{nd} double + {ns} single blocks, image tokens {Li} + text {Lt} (valid {tv.tolist()}), "
                                             "d 3072, 24 x 128, " + ("block weights frozen, rank-4 adapters on the image stream's q / k / v / out projections trained (configs/007 recipe), "
                                                                  if lora else "all block weights trained, ") + "flow-matching loss",
                                 "mode": "lora" if lora else "fullft", "parallelism": f"dp{n_dp} x sp{sp_deg} (Ulysses)" if sp_deg > 1 else f"dp{n_dp}",
                                 "micro_batch": B, "double_blocks": nd, "single_blocks": ns, "weights": "seeded random init"},
                      "peak_hbm_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 1), "step_tflops_algorithmic": step_tf * args.steps / elapsed,
                      **({"kernels": kern} if args.full else {}), "loss_first": lv[0], "loss_last": lv[-1],
                      **({"fp8": {"mode": "every Linear of the double / single blocks holds its weight as E4M3 with a per-tensor scale and multiplies the "
                                          "de-quantised copy in bf16 (the reference's fp8_optimization.py:55-101); activations, gradients and the product stay bf16",
                                  **(fp8_cmp or {})}} if args.fp8 else {})}), flush=True)
    if world > 1:
        dist.barrier(); dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--micro-batch", type=int, default=None, help="default: 4 (2B LoRA), 2 otherwise; vc2 / stdit: 4")
    ap.add_argument("--accum", type=int, default=None, help="default: 1 (2B LoRA), 2 otherwise; vc2 / stdit: 1")
    ap.add_argument("--layers", type=int, default=30, help="debug only; anything but 30 is not the benchmark")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out the CPU-oracle baseline")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: HIP-event times of the attention / GEMM / convolution launches "
                         "in the timed steps (kernels, roofline, roofline_more), the CPU-oracle baseline, the --fp8 line's bf16 loss")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32, at most 64 MB; an "
                         "array of more than 5 M elements as a fixed, seeded sample of its elements); CogVideoX lines (--model 2b / 5b)")
    ap.add_argument("--model", choices=["2b", "5b", "vc2", "stdit", "hunyuan"], default="2b",
                    help="2b = the benchmark (BASELINE configs[1]); 5b = CogVideoX-5B dimensions (48 heads, 42 layers, rotary q/k) -- "
                         "extra data point, labelled as such, never the headline line; vc2 = BASELINE configs[3], the VideoCrafter2 "
                         "320x512 UNet (full fine-tune of 1.41 B weights, latents [4,4,16,40,64]) -- its own metric line")
    ap.add_argument("--text-encoder", action="store_true",
                    help="extra data point: the frozen T5-XXL encoder (vt355.t5, random weights) produces every micro-batch's text "
                         "embeddings inside the loop, one step ahead on a side stream (SURVEY 8(f) row 1); default: pre-encoded text")
    ap.add_argument("--vae-encoder", action="store_true",
                    help="extra data point: every sample's latents come from the CogVideoX VAE encoder (vt355.vae, random weights) run on a "
                         "raw [3,49,480,720] clip inside the loop, one step ahead on a side stream -- the reference encodes online "
                         "(cogvideo_pl.py:792-813); default: pre-encoded latents")
    ap.add_argument("--mode", choices=["lora", "fullft"], default="lora",
                    help="lora = BASELINE configs[1] (the headline metric); fullft = configs[2], every weight trainable")
    ap.add_argument("--fp8", action="store_true", help="--model hunyuan: the reference's fp8 mode (every block Linear's weight E4M3 with a per-tensor "
                                                      "scale, de-quantised for a bf16 product); the line also carries the loss of the same first batch in bf16")
    ap.add_argument("--sp", type=int, default=1, help="--model hunyuan: Ulysses sequence-parallel degree (ranks per sample); --gpus / --sp samples run data parallel")
    ap.add_argument("--latent", default="5,68,120", help="--model hunyuan: latent T,H,W (5,68,120 = the shipped 544x960x17f recipe; 33,90,160 = 720p x 129 frames)")
    ap.add_argument("--encoder-cache", type=int, default=0, metavar="N",
                    help="with --vae-encoder / --text-encoder: the batches cycle through a synthetic dataset of N samples and the frozen encoders' "
                         "outputs are kept per sample (vt355.prefetch.EncodingCache: prompt embeddings by caption, latent MOMENTS by index, the "
                         "sample re-drawn on every hit) -- steady-state epochs then skip the encoders; run with --warmup >= N / (micro_batch * accum)")
    ap.add_argument("--allreduce-dtype", choices=["fp32", "bf16"], default="bf16",
                    help="full fine-tuning, N > 1: wire format of the gradient all-reduce (bf16 = the reference's DDP, whose gradients are "
                         "bf16: 3.4 GB per step; fp32 = the engine's accumulators as they are: 6.8 GB)")
    ap.add_argument("--rehearse", action="store_true",
                    help="no GPU work: the ranks only rendezvous (gloo), all-reduce one number and rank 0 prints it -- the CPU test "
                         "of the launcher / rank plumbing (tests/test_ddp_cpu.py)")
    args = ap.parse_args()
    args.mode_given = any(a == "--mode" or a.startswith("--mode=") for a in sys.argv[1:])
    if args.model in ("2b", "5b"):                       # vc2 / stdit resolve their own defaults
        lora_2b = args.model == "2b" and args.mode == "lora" and not (args.text_encoder or args.vae_encoder)
        if args.micro_batch is None:
            args.micro_batch = 4 if lora_2b else 2
        if args.accum is None:
            args.accum = (4 // args.micro_batch if args.micro_batch in (1, 2, 4) and lora_2b else 2)

    if args.dump_outputs and args.model not in ("2b", "5b"):
        ap.error("--dump-outputs is implemented for the CogVideoX lines (--model 2b / 5b)")
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.rehearse:
        from vt355.ddp import init_from_env
        if os.environ.get("VT_REHEARSE_FAIL_RANK") == os.environ.get("RANK", "0"):
            sys.exit(3)                          # test hook: a rank that dies before the rendezvous
        rank, local, world = init_from_env("gloo")
        assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
        tt = torch.tensor([float(rank + 1)])
        if world > 1:
            dist.all_reduce(tt)
            dist.barrier()
        out = {"rehearsal": True, "n_gpus": world, "rank_sum": tt.item(), "local_rank": local}
        if args.model == "hunyuan" and args.sp > 1:
            # the group construction and sequence-parallel geometry of bench_hunyuan, without a device: every rank creates every group in
            # the same order; the denoiser at its real width (3072 = 24 heads x 128, one double + one single block) takes its group
            from vt355.hunyuan import HYVideoDiffusionTransformer
            sp_deg = args.sp
            assert world % sp_deg == 0, (world, sp_deg)
            n_dp, dp_idx = world // sp_deg, rank // sp_deg
            groups = [dist.new_group(list(range(i * sp_deg, (i + 1) * sp_deg))) for i in range(n_dp)]
            m = HYVideoDiffusionTransformer(mm_double_blocks_depth=1, mm_single_blocks_depth=1, lora_rank=4)
            m.set_sequence_parallel(groups[dp_idx])
            lT, lH, lW = (int(v) for v in args.latent.split(","))
            Li = lT * (lH // 2) * (lW // 2)
            lo, nl = m._sp_rows(Li)
            gs = torch.tensor([float(rank)])
            dist.all_reduce(gs, group=groups[dp_idx])
            mine = {"rank": rank, "sample": dp_idx, "group_rank": dist.get_rank(groups[dp_idx]), "heads_per_rank": m.heads_num // sp_deg,
                    "rows": [lo, nl], "group_rank_sum": gs.item()}
            allr = [None] * world
            dist.all_gather_object(allr, mine)
            out["sp"] = {"degree": sp_deg, "image_tokens": Li, "ranks": allr}
        if rank == 0:
            print(json.dumps(out), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return

    if args.model == "vc2":
        return bench_vc2(args)
    if args.model == "stdit":
        return bench_stdit(args)
    if args.model == "hunyuan":
        return bench_hunyuan(args)

    from vt355 import ops
    from vt355.ddp import BucketedReducer, FlatGradReducer, broadcast_flat, init_from_env
    from vt355.fullft import enable_full_finetune
    from vt355.dit import CogVideoXTransformer3DModel
    from vt355.lora import LoraConfig, get_peft_model
    from vt355.optim import FusedAdamW
    from vt355.scheduler import CogVideoXDPMScheduler
    from vt355.workflow import _LossFn

    # VT_DDP_BACKEND=gloo + VT_ONE_GPU=1 rehearse the multi-rank control flow on a single-GPU box (tests only)
    rank, local, world = init_from_env(os.environ.get("VT_DDP_BACKEND"))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    if os.environ.get("VT_ONE_GPU") == "1":
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    # ---- model: CogVideoX-2B architecture, seeded random init, identical on every rank ----
    if args.model == "5b":
        model = CogVideoXTransformer3DModel(num_layers=42 if args.layers == 30 else args.layers, num_attention_heads=48,
                                            use_rotary_positional_embeddings=True)
    else:
        model = CogVideoXTransformer3DModel(num_layers=args.layers)
    model.to(dev)
    rope = None
    if args.model == "5b":
        from vt355.rope import prepare_rotary_positional_embeddings
        rope = prepare_rotary_positional_embeddings(480, 720, 13, device=dev)        # cogvideo_pl.py:846-859
    gen = torch.Generator(device=dev).manual_seed(1234)
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.normal_(0.0, 0.02, generator=gen)
            if name.endswith(("norm.weight", "norm_final.weight", "norm_q.weight", "norm_k.weight")):
                p.add_(1.0)
    lr = 6e-6 * world * 2                           # scripts/train.py:180-185  lr = world * bs * base_lr (the YAML's batch_size 2)
    if args.mode == "lora":
        model.requires_grad_(False)
        peft = get_peft_model(model, LoraConfig(r=4, lora_alpha=1.0, target_modules=["to_k", "to_q", "to_v", "to_out.0"]))
        st = peft._lora_state
        broadcast_flat(st.flat); st.mark_changed()
        opt = FusedAdamW(st.params, lr=lr, lora_state=st)
        red = FlatGradReducer(st.grad)
    else:
        peft = model
        st = enable_full_finetune(model)
        opt = FusedAdamW(st.params, lr=lr, fullft_state=st)
        red = BucketedReducer(st.grad, wire_dtype=torch.bfloat16 if args.allreduce_dtype == "bf16" else None)
    sched = CogVideoXDPMScheduler()

    B, Fr, C, Hh, Ww, St = args.micro_batch, 13, 16, 60, 90, 226
    dgen = torch.Generator(device=dev).manual_seed(20230211 + rank)      # per-rank data / in-step RNG

    t5 = side = None
    if args.text_encoder:
        from vt355.t5 import T5EncoderModel
        with torch.device(dev):
            t5 = T5EncoderModel()                       # T5 v1.1 XXL dimensions
        with torch.no_grad():
            for name, p in t5.named_parameters():
                p.normal_(0.0, 0.006 if (".q.weight" in name or ".k.weight" in name) else 0.02, generator=gen)
                if name.endswith("layer_norm.weight"):
                    p.add_(1.0)
        side = torch.cuda.Stream(device=dev)

    vae = None
    if args.vae_encoder:
        from vt355.vae import CogVideoXVaeEncoder
        with torch.device(dev):
            vae = CogVideoXVaeEncoder()
        with torch.no_grad():
            for name, p in vae.named_parameters():
                if p.dim() > 1:
                    p.normal_(0.0, 1.0 / p[0].numel() ** 0.5, generator=gen)
                elif name.endswith("weight"):
                    p.fill_(1.0)
                else:
                    p.zero_()
        if side is None:
            side = torch.cuda.Stream(device=dev)

    if side is not None:
        ops.declare_side_stream(True)       # encoder kernels share the CUs with the backward: no dQ hand-off chains (plain atomics)

    ecache, ecount, missing = None, [0], [False]
    if args.encoder_cache > 0 and side is not None:
        from vt355.prefetch import EncodingCache
        ecache = EncodingCache()

    class _LazyClips:                                   # sample i's clip is only materialised when the cache misses it
        def __init__(self, idx): self.idx = idx
        def __getitem__(self, n):
            g = torch.Generator(device=dev).manual_seed(1000 + self.idx[n])
            return torch.rand(3, 49, 480, 720, device=dev, generator=g).mul_(2).sub_(1).to(torch.bfloat16)

    def make_batch_cached():
        """dataset of N samples, index-cycled; misses run the encoders on the side stream (and keep the dQ chains off), hits only draw the sample"""
        N = args.encoder_cache
        idx = [(ecount[0] + b) % N for b in range(B)]
        ecount[0] += B
        miss = (vae is not None and any(i not in ecache.moments for i in idx)) or (t5 is not None and any(f"prompt {i}" not in ecache.text for i in idx))
        missing[0] |= bool(miss)
        stream = side if miss else torch.cuda.current_stream()
        if miss:
            side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            if vae is not None:
                x0 = ecache.latents(idx, _LazyClips(idx), lambda v: vae.encode(v).latent_dist, vae.config.scaling_factor)
                x0 = x0.permute(0, 2, 1, 3, 4).contiguous()
            else:
                x0 = torch.randn(B, Fr, C, Hh, Ww, device=dev, generator=dgen)
            if t5 is not None:
                def enc(caps):
                    ids = torch.stack([torch.randint(0, 32128, (St,), device=dev, generator=torch.Generator(device=dev).manual_seed(int(c.split()[1])))
                                       for c in caps])
                    return t5(ids)[0]
                text = ecache.prompt_embeds([f"prompt {i}" for i in idx], enc)
            else:
                text = (torch.randn(B, St, 4096, device=dev, generator=dgen) * 0.2).to(torch.bfloat16)
            ev = torch.cuda.Event(); ev.record(stream)
        noise = torch.randn(B, Fr, C, Hh, Ww, device=dev, generator=dgen)
        t = torch.randint(0, 1000, (B,), device=dev, generator=dgen)
        return (x0, ev), (text, ev), noise, t

    def make_batch():
        if ecache is not None:
            return make_batch_cached()
        if vae is not None:                             # raw clips -> frozen VAE encoder on the side stream, sample by sample
            clips = torch.rand(B, 3, 49, 480, 720, device=dev, generator=dgen).mul_(2).sub_(1).to(torch.bfloat16)
            clips.record_stream(side)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                lat = [vae.encode(clips[b:b + 1]).latent_dist.sample() * vae.config.scaling_factor for b in range(B)]
                x0 = torch.cat(lat, 0).permute(0, 2, 1, 3, 4).contiguous()          # [B,C,F,H,W] -> [B,F,C,H,W] (cogvideo_pl.py:817-819)
                ev_x = torch.cuda.Event(); ev_x.record(side)
            x0 = (x0, ev_x)
        else:
            x0 = torch.randn(B, Fr, C, Hh, Ww, device=dev, generator=dgen)
        if t5 is not None:                              # token ids -> frozen encoder on the side stream; the DiT waits on the event
            ids = torch.randint(0, 32128, (B, St), device=dev, generator=dgen)
            side.wait_stream(torch.cuda.current_stream())
            ids.record_stream(side)                     # allocated on the main stream, consumed on the side stream
            with torch.cuda.stream(side):
                text = t5(ids)[0]
                ev = torch.cuda.Event(); ev.record(side)
            text = (text, ev)
        else:
            text = (torch.randn(B, St, 4096, device=dev, generator=dgen) * 0.2).to(torch.bfloat16)
        noise = torch.randn(B, Fr, C, Hh, Ww, device=dev, generator=dgen)
        t = torch.randint(0, 1000, (B,), device=dev, generator=dgen)
        return x0, text, noise, t

    batches = [make_batch() for _ in range(args.accum)]
    losses = []
    last = {} if args.dump_outputs else None       # --dump-outputs: the prediction of the step's last micro-batch

    def step():
        nonlocal batches
        nxt = None
        if t5 is not None or vae is not None:     # the NEXT step's prompts / clips are encoded while this step's DiT runs
            missing[0] = False
            nxt = [make_batch() for _ in range(args.accum)]
            if ecache is not None:                # encoder kernels run beside this step's backward only when the cache missed
                ops.declare_side_stream(missing[0])
        opt.zero_grad()
        for mb in range(args.accum):
            x0, text, noise, t = batches[mb]
            if isinstance(x0, tuple):
                x0, ev_x = x0
                torch.cuda.current_stream().wait_event(ev_x)
                x0.record_stream(torch.cuda.current_stream())
            if isinstance(text, tuple):
                text, ev = text
                torch.cuda.current_stream().wait_event(ev)
                text.record_stream(torch.cuda.current_stream())
            noisy = sched.add_noise(x0, noise, t)
            out = peft(hidden_states=noisy, encoder_hidden_states=text, timestep=t, image_rotary_emb=rope, return_dict=False)[0]
            sa, sb, w = sched.coefficients(t)
            loss = _LossFn.apply(out, noisy, x0, sa, sb, w)
            if last is not None:
                last["prediction"] = out.detach()
            if args.mode == "fullft":             # DDP no_sync: slices are all-reduced only on the last micro-batch,
                st.on_grads_ready = red.hook if mb == args.accum - 1 else None      # as the backward finishes them
            (loss / args.accum).backward()
            losses.append(loss.detach())
        if args.mode == "lora":
            red.reduce_async()                    # one RCCL all-reduce of the flat LoRA gradient ...
        batches = nxt if nxt is not None else [make_batch() for _ in range(args.accum)]   # ... overlapped with the next step's input generation
        if args.mode == "lora":
            red.wait()
        else:
            covered = red.wait_all()
            assert covered == st.numel, (covered, st.numel)   # every gradient element was reduced exactly once
        opt.step(grad_scale=red.grad_scale)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    ops.profile_reset(args.full)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    elapsed = time.perf_counter() - t0
    prof = ops.profile_collect()
    ops.profile_reset(False)
    assert ops.attn_bwd_chain_errors() == 0, "a dQ hand-off wait of the attention backward timed out: results invalid"
    if world > 1:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = tt.item()
    samples = world * args.micro_batch * args.accum * args.steps
    loss_vals = [float(x) for x in torch.stack(losses[-args.accum * args.steps:]).cpu()]

    if rank == 0:
        S, d = St + Fr * (Hh // 2) * (Ww // 2), model.inner_dim
        alg = {"attn_bwd": 8.0 * S * S * d * B, "attn_fwd": 4.0 * S * S * d * B}     # algorithmic FLOPs per launch
        work = ops.profile_work()
        kern = {}
        hbm_kernels = {"ln_modulate_fwd": "ln_modulate_fwd_kernel (LayerNorm + adaLN shift / scale)", "ln_modulate_bwd": "ln_modulate_bwd_kernel",
                       "qk_layernorm_fwd": "qk_layernorm_fwd_kernel (per-head q / k LayerNorm)", "qk_layernorm_bwd": "qk_layernorm_bwd_kernel",
                       "adamw": "adamw_kernel (fp32 master, moments, bf16 copy)"}
        for name, (ms, n) in prof.items():
            kern[name] = {"avg_ms": ms, "launches": n}
            if name in alg:
                kern[name]["tflops_algorithmic"] = alg[name] / ms / 1e9
            elif name in hbm_kernels:             # memory-bound kernels: the recorded work is algorithmic HBM bytes (SURVEY 8(d) ii)
                kern[name]["gb_per_s_algorithmic"] = work[name] / (ms * n) / 1e6
            elif name in work:
                kern[name]["tflops_algorithmic"] = work[name] / (ms * n) / 1e9
        hbm_lines = [{"bound": "hbm", "kernel": hbm_kernels[name], "achieved": kern[name]["gb_per_s_algorithmic"], "peak": 8000.0, "unit": "GB/s",
                      "frac": kern[name]["gb_per_s_algorithmic"] / 8000.0} for name in hbm_kernels if name in kern and "gb_per_s_algorithmic" in kern[name]]
        dom = "attn_bwd"
        ach = kern[dom]["tflops_algorithmic"] if dom in kern else None
        # HBM bytes per launch of the dominant kernel: PMC counters cannot be read from inside the process, so the figure comes from
        # the committed rocprofv3 --pmc summary of this same command (tools/pmc_bench.sh), corrected as MI355X_MICROARCH.md
        # prescribes (FETCH_SIZE x2 on gfx950, KiB units).  The summary records the hash of the kernel source it was measured on: a
        # figure from another version of the kernel is NOT quoted (traffic = null).
        traffic, traffic_note = None, "no PMC summary for this kernel source"
        try:
            import hashlib
            src = hashlib.sha256(open(os.path.join(ROOT, "videotuna-dev_amd", "csrc", "attn_bwd.hip"), "rb").read()).hexdigest()[:16]
            import glob as _glob
            alg_gb = 8 * args.micro_batch * S * 30 * 64 * 2 / 1e9       # q, k, v, o, dO read + dQ, dK, dV written, bf16
            for path in (sorted(_glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_bench_summary.json")), reverse=True) if args.full else []):
                with open(path) as f:
                    summ = json.load(f)
                rel = os.path.relpath(path, ROOT)
                if summ.get("provenance", {}).get("attn_bwd_src_sha16") != src:
                    traffic_note = rel + " was measured on another version of attn_bwd.hip: not quoted"
                    continue
                if args.micro_batch == summ.get("provenance", {}).get("micro_batch", 2) and args.layers == 30 and args.model == "2b":
                    key = [k for k in summ["traffic"] if "attn_bwd_hd64_kernel" in k][0]
                    traffic = summ["traffic"][key]["hbm_bytes_per_launch"]
                    traffic_note = ("bytes/launch, rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE (%s, same kernel source %s); algorithmic "
                                    "bytes are %.1f GB at micro-batch %d, the rest are the fp32 dQ atomics and hand-off tiles"
                                    % (rel, src, alg_gb, args.micro_batch))
                break
        except Exception:
            traffic = None
        from vt355 import engine as _eng
        _kept = _eng.saved_bytes_per_block(model, args.micro_batch * S) * model.config.num_layers / 1e9
        recompute_note = ("per block (VT355_RECOMPUTE / enable_gradient_checkpointing: activations rebuilt in the backward pass)"
                          if _eng._use_recompute(model, (args.micro_batch * S,)) else
                          "none (%.0f GB of block activations kept in HBM)" % _kept)
        res = {
            "metric": "finetune samples/sec, CogVideoX-%s T2V %s 49x480x720 bf16" % ("2B" if args.model == "2b" else "5B",
                                                                                       "LoRA" if args.mode == "lora" else "full-FT"),
            "value": samples / elapsed,
            "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1000.0 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": {"workload": ("CogVideoX-2B T2V LoRA finetune 49x480x720 (configs[1]): latents [%d,13,16,60,90], text [%d,226,4096], r=4 LoRA on "
                                    "to_q/k/v/out, 4 samples per optimizer step as in the YAML (batch_size 2 x accumulate_grad_batches 2), run as "
                                    "%d micro-batch(es) of %d" % (args.micro_batch, args.micro_batch, args.accum, args.micro_batch)) if args.mode == "lora" else
                                   ("CogVideoX-2B T2V FULL finetune 49x480x720 (configs[2]): all 1.69 B weights trainable, fp32 master "
                                    "+ fused AdamW, per-block gradient slices all-reduced under the backward"),
                       "mode": args.mode, "model": "CogVideoX-" + args.model.upper() + ("" if args.model == "2b" else
                                                                                          " (NOT the benchmark config: extra data point)"),
                       "micro_batch": args.micro_batch, "accumulate_grad_batches": args.accum,
                       "global_batch": world * args.micro_batch * args.accum, "seq_len": S, "layers": model.config.num_layers,
                       "parallelism": f"dp{world}", "recompute": recompute_note,
                       "weights": "seeded random init (no checkpoints offline)",
                       "text": ("T5-XXL encoder (vt355.t5, random weights) in the loop, one step ahead on a side stream"
                                if args.text_encoder else "pre-encoded prompt embeddings (synthetic)"),
                       "latents": ("CogVideoX VAE encoder (vt355.vae, random weights) on raw 49x480x720 clips in the loop, one step ahead "
                                   "on a side stream" if args.vae_encoder else "pre-encoded latents (synthetic)"),
                       **({"encoder_cache": {"dataset": args.encoder_cache, "hits": dict(ecache.hits), "misses": dict(ecache.misses)}} if ecache is not None else {})},
            "peak_hbm_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 1),
            "ddp": {"backend": (dist.get_backend() if world > 1 else None), "world_size_seen": (dist.get_world_size() if world > 1 else 1),
                    "allreduce_bytes_per_step": (int(st.grad.numel() * (2 if (args.mode == "fullft" and args.allreduce_dtype == "bf16") else 4)) if world > 1 else 0),
                    "allreduce_dtype": (args.allreduce_dtype if args.mode == "fullft" else "fp32"),
                    "dq_chains": bool(ops.attn_bwd_chain_workspace(args.micro_batch, model.config.num_attention_heads, S, dev) is not None)},
            "loss_last": loss_vals[-1], "loss_first": loss_vals[0],
        }
        if args.dump_outputs:        # rank 0's last timed step: its losses, the last micro-batch's prediction, the updated weights, the gradient
            res["outputs"] = dump_outputs(args.dump_outputs, {"loss": torch.stack(losses[-args.accum:]), "prediction": last["prediction"],
                                                              "params": st.flat, "grads": st.grad})
        if args.full:
            res["roofline"] = {"bound": "mfma", "kernel": "attn_bwd_hd64_kernel", "achieved": ach, "peak": 2500.0,
                               "unit": "TFLOP/s", "frac": (ach / 2500.0) if ach else None, "traffic": traffic,
                               "traffic_unit": traffic_note,
                               "note": "algorithmic FLOPs per launch 8*S^2*d*B (dQ,dK,dV products; P recompute not counted)"}
            res["roofline_more"] = [
                {"bound": "mfma", "kernel": "attn_fwd_hd64_kernel", "achieved": kern.get("attn_fwd", {}).get("tflops_algorithmic"), "peak": 2500.0,
                 "unit": "TFLOP/s", "frac": (kern["attn_fwd"]["tflops_algorithmic"] / 2500.0) if "attn_fwd" in kern else None},
                {"bound": "mfma", "kernel": "gemm_tn_* (every Linear with >= 4096 rows, forward and dX)", "achieved": kern.get("gemm", {}).get("tflops_algorithmic"),
                 "peak": 2500.0, "unit": "TFLOP/s", "frac": (kern["gemm"]["tflops_algorithmic"] / 2500.0) if kern.get("gemm", {}).get("tflops_algorithmic") else None}] + hbm_lines
            res["kernels"] = kern
            if world == 1 and not args.no_cpu_baseline:
                res["cpu_baseline"] = cpu_baseline()
        print(json.dumps(res), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
