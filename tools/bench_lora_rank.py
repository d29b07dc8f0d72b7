"""What a higher LoRA rank costs in the training step: the CogVideoX-2B LoRA step of ``bench.py``'s default line (49x480x720, bf16, one
micro-batch of 4 samples, adapters on to_q / to_k / to_v / to_out.0, fused AdamW) at ranks 4, 16, 64 and 128 in ONE process on one box.
Each rank has its own model (same seeded base weights); blocks of --steps steps alternate over the ranks for --rounds rounds, so drift
of the box hits every rank alike.  Prints one JSON line: per rank the median ms per step with its spread over the rounds, the peak HBM
of its blocks (the other ranks' idle models, ~3.4 GB of weights each, are resident and counted) and the step-time delta against rank 4
of the same run.  Ranks <= 16 run the narrow rank-side kernels (csrc/lora.hip), 64 and 128 the MFMA ones (csrc/lora_wide.hip).
--lora-dropout P (> 0) times every rank twice, lora_dropout = 0 and = P on the same model, alternating block by block: the entry
"<rank>+drop" carries the delta against the same rank without dropout (the _drop kernels recompute a Philox mask in every pass).

    python tools/bench_lora_rank.py [--ranks 4,16,64,128] [--rounds 3] [--steps 2] [--warmup 1] [--micro-batch 4] > profiles/lora_rank_step.json
--targets attn,attn+ff times every rank with the adapters on the four attention projections and again with ff.net.0.proj / ff.net.2
added (a model each; the entry "<rank>+ff" carries the delta against the same rank and dropout setting without the feed-forward pair).

    python tools/bench_lora_rank.py --ranks 4,64 --lora-dropout 0.1 > profiles/lora_dropout_step.json
    python tools/bench_lora_rank.py --ranks 4,64 --targets attn,attn+ff --lora-dropout 0.1 > profiles/lora_ff_step.json
--use-dora times every rank as LoRA and again with use_dora=True (a model each: the flat layouts differ; the blocks alternate like the
others): the entry "<rank>+dora" carries the delta against the same rank and targets without DoRA, and both carry "repack_ms", the
time of engine.packed() right after an adapter version bump (LoRA: the pack kernels; DoRA: those, the row norms and the scaled
refresh of every operand) -- part of every step, measured alone.

    python tools/bench_lora_rank.py --ranks 4,64 --use-dora > profiles/lora_dora_step.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", default="4,16,64,128")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--micro-batch", type=int, default=4)
    ap.add_argument("--lora-dropout", type=float, default=0.0, help="P > 0: time lora_dropout = 0 and = P per rank, alternating")
    ap.add_argument("--targets", default="attn", help="comma list of attn | attn+ff: the adapted Linears (attn+ff adds ff.net.0.proj, ff.net.2)")
    ap.add_argument("--use-dora", action="store_true", help="time every rank with use_dora False and True, alternating")
    ap.add_argument("--layers", type=int, default=30, help="debug only; anything but 30 is not the benchmark's model")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from vt355 import ops
    from vt355.dit import CogVideoXTransformer3DModel
    from vt355.lora import LoraConfig, get_peft_model
    from vt355.optim import FusedAdamW
    from vt355.scheduler import CogVideoXDPMScheduler
    from vt355.workflow import _LossFn
    if not torch.cuda.is_available():
        raise SystemExit("bench_lora_rank needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    ranks = [int(v) for v in args.ranks.split(",")]
    ATTN = ["to_k", "to_q", "to_v", "to_out.0"]
    target_sets = {"attn": ATTN, "attn+ff": ATTN + ["ff.net.0.proj", "ff.net.2"]}
    tsets = args.targets.split(",")
    if any(t not in target_sets for t in tsets):
        raise SystemExit(f"--targets takes a comma list of {sorted(target_sets)}")
    B, Fr, C, Hh, Ww, St = args.micro_batch, 13, 16, 60, 90, 226
    sched = CogVideoXDPMScheduler()
    dgen = torch.Generator(device=dev).manual_seed(20230211)

    runs = {}
    for r, ts, dora in [(r, ts, dora) for r in ranks for ts in tsets for dora in ([False, True] if args.use_dora else [False])]:
        model = CogVideoXTransformer3DModel(num_layers=args.layers).to(dev)
        gen = torch.Generator(device=dev).manual_seed(1234)            # bench.py's weights
        with torch.no_grad():
            for name, p in model.named_parameters():
                p.normal_(0.0, 0.02, generator=gen)
                if name.endswith(("norm.weight", "norm_final.weight", "norm_q.weight", "norm_k.weight")):
                    p.add_(1.0)
        model.requires_grad_(False)
        peft = get_peft_model(model, LoraConfig(r=r, lora_alpha=r / 4.0, target_modules=target_sets[ts], use_dora=dora))
        st = peft._lora_state
        key = str(r) + ts[4:] + ("+dora" if dora else "")          # "4", "4+ff", "4+dora"
        runs[key] = dict(peft=peft, st=st, opt=FusedAdamW(st.params, lr=1.2e-5, lora_state=st), ms=[], peak=0.0, loss=None, p=0.0, rank=r,
                         targets=ts, model=model)
        if args.lora_dropout > 0 and not dora:
            LoraConfig(r=r, lora_dropout=args.lora_dropout)        # validates P
            runs[f"{key}+drop"] = dict(runs[key], ms=[], p=args.lora_dropout)

    def step(run):
        x0 = torch.randn(B, Fr, C, Hh, Ww, device=dev, generator=dgen)
        text = (torch.randn(B, St, 4096, device=dev, generator=dgen) * 0.2).to(torch.bfloat16)
        noise = torch.randn(B, Fr, C, Hh, Ww, device=dev, generator=dgen)
        t = torch.randint(0, 1000, (B,), device=dev, generator=dgen)
        run["st"].p = run["p"]
        run["opt"].zero_grad()
        noisy = sched.add_noise(x0, noise, t)
        out = run["peft"](hidden_states=noisy, encoder_hidden_states=text, timestep=t, return_dict=False)[0]
        sa, sb, w = sched.coefficients(t)
        loss = _LossFn.apply(out, noisy, x0, sa, sb, w)
        loss.backward()
        run["opt"].step()
        run["loss"] = loss.detach()

    for run in runs.values():
        for _ in range(args.warmup):
            step(run)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for run in runs.values():
            torch.cuda.reset_peak_memory_stats(dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(run)
            torch.cuda.synchronize()
            run["ms"].append(1000.0 * (time.perf_counter() - t0) / args.steps)
            run["peak"] = max(run["peak"], torch.cuda.max_memory_allocated(dev) / 1e9)
    assert ops.attn_bwd_chain_errors() == 0, "a dQ hand-off wait of the attention backward timed out: results invalid"
    res = {"metric": "CogVideoX-2B T2V LoRA step 49x480x720 bf16 by adapter rank, same process, alternating", "unit": "ms per step",
           "micro_batch": B, "layers": args.layers, "rounds": args.rounds, "steps_per_block": args.steps, "warmup_per_rank": args.warmup,
           "device": torch.cuda.get_device_name(0), "ranks": {}}
    base = statistics.median(runs[str(ranks[0]) + tsets[0][4:]]["ms"])
    for key, run in runs.items():
        st = run["st"]
        med = statistics.median(run["ms"])
        res["ranks"][key] = {"median_ms": round(med, 2), "spread_ms": round(max(run["ms"]) - min(run["ms"]), 2),
                                "rounds_ms": [round(v, 2) for v in run["ms"]], "samples_per_s": round(B / (med / 1e3), 3),
                                "peak_hbm_gb_all_models_resident": round(run["peak"], 1),
                                "layout": {"wide": st.wide, "rp": st.rp, "ext_qkv": st.ext_qkv, "ext_o": st.ext_o}, "targets": run["targets"],
                                "trainable_params": st.flat.numel(), "loss_last": float(run["loss"]),
                                f"delta_vs_r{ranks[0]}_ms": round(med - base, 2), f"delta_vs_r{ranks[0]}_pct": round(100.0 * (med - base) / base, 2)}
        if run["targets"] == "attn+ff":
            from vt355 import engine
            res["ranks"][key]["saved_gb_per_block"] = round(engine.saved_bytes_per_block(run["model"], B * (St + Fr * (Hh // 2) * (Ww // 2))) / 1e9, 3)
            # what enable_gradient_checkpointing("auto") would choose for this model here (engine._use_recompute: keep while the saved
            # activations stay under 0.6 of the free HBM); the timed steps themselves keep everything
            free = torch.cuda.mem_get_info()[0] / 1e9
            need = res["ranks"][key]["saved_gb_per_block"] * args.layers
            res["ranks"][key].update({"saved_gb_all_blocks": round(need, 1), "free_hbm_gb_after_run": round(free, 1),
                                      "auto_recompute_would": "recompute" if need > 0.6 * free else "keep"})
            if "attn" in tsets:
                same =statistics.median(runs[str(run["rank"]) + ("+drop" if run["p"] > 0 else "")]["ms"])
                res["ranks"][key].update({"delta_vs_attn_only_ms": round(med - same, 2), "delta_vs_attn_only_pct": round(100.0 * (med - same) / same, 2)})
        if args.use_dora and run["p"] == 0:
            from vt355 import engine
            times = []
            for _ in range(3):
                st.version += 1
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                engine.packed(run["model"])
                torch.cuda.synchronize()
                times.append(1000.0 * (time.perf_counter() - t0))
            res["ranks"][key]["repack_ms"] = round(statistics.median(times), 2)
            if st.dora:
                same = statistics.median(runs[key[:-5]]["ms"])
                res["ranks"][key].update({"use_dora": True, "delta_vs_lora_ms": round(med - same, 2),
                                          "delta_vs_lora_pct": round(100.0 * (med - same) / same, 2),
                                          "spread_of_lora_ms": round(max(runs[key[:-5]]["ms"]) - min(runs[key[:-5]]["ms"]), 2)})
        if run["p"] > 0:
            same = statistics.median(runs[key[:-5]]["ms"])
            res["ranks"][key].update({"lora_dropout": run["p"], "delta_vs_no_dropout_ms": round(med - same, 2),
                                      "delta_vs_no_dropout_pct": round(100.0 * (med - same) / same, 2)})
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
