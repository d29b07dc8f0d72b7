"""Same-box A/B of HunyuanVideo's fp8 modes on the workload of ``bench.py --model hunyuan``: the whole HYVideoDiffusionTransformer (20 double
+ 40 single blocks, d 3072, 24 x 128), latents [1, 16, 5, 68, 120] (10 200 image tokens) + 256 text tokens, rank-4 LoRA, through
HunyuanVideoFlow.training_step with backward and optimizer step.

A model needs 126-151 GB, so two cannot share a card: every (mode, round) runs in a child process of its own, under its own time limit,
and the modes alternate (False, "weights", "mfma", "mfma+dgrad", "mfma+dgrad-e4m3", False, ...) for ``--rounds`` rounds.  A child that
fails ends the run (no retries).  "mfma+dgrad" / "mfma+dgrad-e4m3": fp8="mfma" with the input-gradient products on the fp8 matrix cores
too (fp8_dgrad, gradients quantised to E5M2 / E4M3).
The parent prints ONE JSON line: per mode the median and spread (max - min) of the rounds' ms/step and the loss on the bench's fixed batch
(fixed sigma / noise draws, ``loss_only`` of bench.py), plus the relative step-time and loss deltas of "mfma" vs bf16 and, per dgrad mode,
of that mode vs "mfma" in the same run (``dgrad_vs_mfma``: is the median below "mfma"'s by more than the larger of the two spreads?).

Weights: seeded random init drawn on the device (the same for every mode; the CPU draw of bench.py takes minutes per child at this size).

    python tools/bench_hunyuan_fp8_ab.py [--rounds 3] [--steps 4] [--warmup 2] [--timeout 900] [--modes bf16,mfma,mfma+dgrad]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"bf16": False, "weights": "weights", "mfma": "mfma", "mfma+dgrad": "mfma", "mfma+dgrad-e4m3": "mfma"}
DGRAD = {"mfma+dgrad": "e5m2", "mfma+dgrad-e4m3": "e4m3"}


def child(mode: str, steps: int, warmup: int):
    sys.path.insert(0, ROOT)
    import torch
    from vt355.hunyuan import HYVideoDiffusionTransformer, HunyuanVideoFlow
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    B, Lt, (lT, lH, lW) = 1, 256, (5, 68, 120)
    model = HYVideoDiffusionTransformer(mm_double_blocks_depth=20, mm_single_blocks_depth=40, lora_rank=4, fp8=MODES[mode],
                                        fp8_dgrad=DGRAD.get(mode, False)).to(dev)
    g = torch.Generator(device=dev).manual_seed(11)
    with torch.no_grad():                     # HunyuanBlocks.init_weights' distribution, drawn on the device
        for n, p in model._plist.items():
            s = model.shapes[n]
            if len(s) == 1:
                p.copy_(torch.randn(s, device=dev, generator=g) * 0.05 + (1.0 if "norm.weight" in n else 0.0))
            else:
                p.copy_(torch.randn(s, device=dev, generator=g) * (0.7 / s[1] ** 0.5))
    model._packed = None
    model.lora.init_weights(12, zero_b=False)
    flow = HunyuanVideoFlow(model=model, learning_rate=1e-5).to(dev)
    opt = flow.configure_optimizers()
    tv = torch.tensor([Lt - 37 * (b % 5) for b in range(B)], device=dev)
    mask = (torch.arange(Lt, device=dev)[None, :] < tv[:, None]).long()

    def make_batch(gen):
        return {"latents": torch.randn(B, 16, lT, lH, lW, device=dev, generator=gen),
                "prompt_embeds": torch.randn(B, Lt, 4096, device=dev, generator=gen).to(torch.bfloat16), "prompt_attention_mask": mask,
                "pooled_prompt_embeds": torch.randn(B, 768, device=dev, generator=gen).to(torch.bfloat16)}

    gb = torch.Generator(device=dev).manual_seed(20230211)
    losses = []

    def step():
        loss = flow.training_step(make_batch(gb))
        loss.backward()
        losses.append(loss.detach())
        opt.step()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = 1000.0 * (time.perf_counter() - t0) / steps
    torch.manual_seed(4242)
    with torch.no_grad():
        l_fixed = float(flow.training_step(make_batch(torch.Generator(device=dev).manual_seed(99))))
    print("AB " + json.dumps({"mode": mode, "ms_per_step": ms, "loss_fixed_batch": l_fixed, "loss_last": float(losses[-1]),
                              "peak_hbm_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=900, help="seconds per child")
    ap.add_argument("--child", choices=list(MODES), default=None)
    ap.add_argument("--modes", default=",".join(MODES), help="comma-separated subset of " + ", ".join(MODES) + " (bf16 and mfma always run)")
    args = ap.parse_args()
    if args.child:
        child(args.child, args.steps, args.warmup)
        return
    chosen = set(args.modes.split(",")) | {"bf16", "mfma"}
    if not chosen <= set(MODES):
        raise SystemExit(f"--modes: unknown {sorted(chosen - set(MODES))}")
    modes = [m for m in MODES if m in chosen]
    runs = {m: [] for m in modes}
    for r in range(args.rounds):
        for mode in modes:
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", mode,
                   "--steps", str(args.steps), "--warmup", str(args.warmup)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("AB ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-3000:] + p.stderr[-3000:])
                raise SystemExit(f"round {r} mode {mode}: child exited {p.returncode}; stopping")
            res = json.loads(line[0][3:])
            runs[mode].append(res)
            print(f"# round {r} {mode}: {res}", file=sys.stderr, flush=True)
    out = {}
    for mode, rs in runs.items():
        ms = [x["ms_per_step"] for x in rs]
        out[mode] = {"ms_per_step_median": statistics.median(ms), "ms_per_step_spread": max(ms) - min(ms), "ms_per_step": ms,
                     "loss_fixed_batch": rs[0]["loss_fixed_batch"], "peak_hbm_gb": max(x["peak_hbm_gb"] for x in rs)}
    b, q = out["bf16"], out["mfma"]
    dg = {}
    for mode in DGRAD:
        if mode in out:
            d = out[mode]
            gain = q["ms_per_step_median"] - d["ms_per_step_median"]
            dg[mode] = {"step_time_rel_delta": d["ms_per_step_median"] / q["ms_per_step_median"] - 1.0, "ms_gain_median": gain,
                        "faster_beyond_spread": gain > max(q["ms_per_step_spread"], d["ms_per_step_spread"]),
                        "loss_fixed_batch_rel_delta_vs_bf16": abs(d["loss_fixed_batch"] - b["loss_fixed_batch"]) / abs(b["loss_fixed_batch"]),
                        "peak_hbm_gb_delta": round(d["peak_hbm_gb"] - q["peak_hbm_gb"], 1)}
    print(json.dumps({"workload": "HYVideoDiffusionTransformer 20 + 40 blocks, latents 1x16x5x68x120 + 256 text tokens, LoRA r 4, "
                                  "HunyuanVideoFlow.training_step + backward + FusedAdamW step",
                      "rounds": args.rounds, "steps": args.steps, "warmup": args.warmup, "modes": out,
                      "mfma_vs_bf16": {"step_time_rel_delta": q["ms_per_step_median"] / b["ms_per_step_median"] - 1.0,
                                       "loss_fixed_batch_rel_delta": abs(q["loss_fixed_batch"] - b["loss_fixed_batch"]) / abs(b["loss_fixed_batch"])},
                      **({"dgrad_vs_mfma": dg} if dg else {})}),
          flush=True)


if __name__ == "__main__":
    main()
