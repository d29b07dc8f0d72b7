"""What a higher LoRA rank costs in the HunyuanVideo training step: the ``bench.py --model hunyuan`` workload (the whole
HYVideoDiffusionTransformer, 20 + 40 blocks, latents 16x5x68x120 = 10 200 image tokens + 256 text tokens, one sample, frozen weights,
adapters on the image stream's q / k / v / out projections, HunyuanVideoFlow.training_step + fused AdamW) at ranks 4, 16, 32, 64 and 128,
in bf16 and in fp8="mfma" + fp8_dgrad, in ONE process on one box.  The frozen denoiser (25.7 GB of bf16 weights) exists once; every rank
has its own adapter set (same seed), optimizer and packed K-extension operands, swapped in as ``model.lora``.  Within a mode, blocks of
--steps steps alternate over the ranks for --rounds rounds, so drift of the box hits every rank alike; the modes run one after the other
(switching the mode rebuilds every packed operand).  Ranks with 3 r <= 64 run the narrow layout, the others the wide one
(vt355.hunyuan.lora_layout).  Prints one JSON line: per mode and rank the median ms per step with its spread over the rounds, the peak
HBM of its blocks (the other ranks' packed operands are resident and counted) and the delta against rank 4 of the same mode.

    python tools/bench_hunyuan_lora_rank.py [--ranks 4,16,32,64,128] [--rounds 3] [--steps 2] [--warmup 1] > profiles/hunyuan_lora_rank_step.json

``--targets attn,attn+ff`` adds the target set as a second axis: ``attn`` = the attention projections (the default, lora_target_modules=None),
``attn+ff`` = all eight targets (ff.net.0.proj, ff.net.2, proj_mlp, proj_out as well); ``ff`` = the four feed-forward targets alone.  Every
(target set, rank) pair is a variant of its own in the alternation; the result then carries the trainable parameters of each and is keyed
"<targets>/<rank>", deltas against the first variant.

    python tools/bench_hunyuan_lora_rank.py --targets attn,attn+ff --ranks 4,64 --modes bf16,mfma,mfma+dgrad > profiles/hunyuan_lora_ff_step.json

``--lora-dropout P`` adds dropout as an axis: per (target set, rank) the variants ``p0`` (lora_dropout 0 in the layout the rank takes by
itself), ``p0-wide`` (lora_dropout 0 in the wide layout, as VT355_LORA_WIDE=1 gives it; the same variant where the rank is wide anyway)
and ``pP`` (lora_dropout P, which takes the wide layout at every rank), alternating like the ranks.  The result then carries, per
rank, the layout switch (p0-wide against p0) and the dropout delta against p0-wide -- two separate costs.  Not with fp8_dgrad.

    python tools/bench_hunyuan_lora_rank.py --ranks 4,64 --modes bf16,mfma --lora-dropout 0.1 > profiles/hunyuan_lora_dropout_step.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODES = {"bf16": (False, False), "mfma": ("mfma", False), "mfma+dgrad": ("mfma", True)}
_ATTN = ["to_q", "to_k", "to_v", "to_out.0"]
_FF = ["ff.net.0.proj", "ff.net.2", "proj_mlp", "proj_out"]
TARGETS = {"attn": None, "attn+ff": _ATTN + _FF, "ff": _FF}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", default="4,16,32,64,128")
    ap.add_argument("--modes", default="bf16,mfma+dgrad")
    ap.add_argument("--targets", default="attn", help="comma-separated target sets: " + ", ".join(TARGETS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--lora-dropout", type=float, default=0.0, help="p > 0: the variants p0 / p0-wide / pP per rank")
    ap.add_argument("--layers", type=int, default=30, help="debug only; anything but 30 is not the benchmark's model")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from vt355.hunyuan import HunyuanVideoFlow, HYVideoDiffusionTransformer, _HYLora
    from vt355.optim import FusedAdamW
    if not torch.cuda.is_available():
        raise SystemExit("bench_hunyuan_lora_rank needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    tsets = args.targets.split(",")
    keyed = tsets != ["attn"]                    # the default keeps the result's rank keys
    # The variants share ONE pack of the frozen weights, built on the first step for the first variant's sites: it holds a bf16 transpose of
    # every Linear that variant does not adapt.  "attn" first serves "attn+ff" too (which needs fewer); "ff" adapts other Linears than it keeps.
    if len(tsets) > 1 and ("ff" in tsets or tsets[0] != "attn"):
        raise SystemExit("--targets: several sets share one weight pack -- put attn first, and run ff in a process of its own")
    ranks = [(tg, int(v)) for tg in tsets for v in args.ranks.split(",")]
    name = lambda k: (f"{k[0]}/{k[1]}" if keyed else str(k[1])) + (f"/{k[2]}" if len(k) > 2 else "")
    pd = args.lora_dropout
    if pd > 0:                                   # (target set, rank, dropout variant)
        ranks = [k + (v,) for k in ranks for v in ("p0", "p0-wide", f"p{pd:g}")]
    nd, ns = (20, 40) if args.layers == 30 else (max(1, args.layers // 3), max(1, args.layers - args.layers // 3))
    lT, lH, lW, Lt, B = 5, 68, 120, 256, 1
    model = HYVideoDiffusionTransformer(mm_double_blocks_depth=nd, mm_single_blocks_depth=ns, lora_rank=ranks[0][1]).to(dev).init_weights(11)
    flow = HunyuanVideoFlow(model=model, learning_rate=1e-5).to(dev)
    runs = {}
    for key in ranks:
        tg, r = key[:2]
        var = key[2] if len(key) > 2 else "p0"
        if var == "p0-wide":
            os.environ["VT355_LORA_WIDE"] = "1"          # read at construction
        L = _HYLora(model.hidden_size, nd, ns, r, 1.0, model.ratio, TARGETS[tg], dropout=pd if var not in ("p0", "p0-wide") else 0.0).to(dev)
        os.environ.pop("VT355_LORA_WIDE", None)
        L.init_weights(12, zero_b=False)
        model.lora = L
        ts = model.enable_lora_training()
        runs[key] = dict(lora=L, opt=FusedAdamW(ts.params, lr=1e-5, fullft_state=ts), layout="wide" if L.wide else "narrow",
                         ext=(L.ext_qkv, L.ext_proj), params=sum(int(torch.tensor(sh).prod()) for sh in L.shapes.values()))
    g = torch.Generator(device=dev).manual_seed(20230211)
    tv = torch.tensor([Lt], device=dev)
    mask = (torch.arange(Lt, device=dev)[None, :] < tv[:, None]).long()

    def step(run):
        model.lora = run["lora"]
        batch = {"latents": torch.randn(B, 16, lT, lH, lW, device=dev, generator=g),
                 "prompt_embeds": torch.randn(B, Lt, 4096, device=dev, generator=g).to(torch.bfloat16), "prompt_attention_mask": mask,
                 "pooled_prompt_embeds": torch.randn(B, 768, device=dev, generator=g).to(torch.bfloat16)}
        loss = flow.training_step(batch)
        loss.backward()
        run["opt"].step()
        run["loss"] = loss.detach()

    out = {}
    for mode in args.modes.split(","):
        fp8, dgrad = MODES[mode]
        model.fp8_dgrad = False
        model.fp8 = fp8
        model.fp8_dgrad = dgrad
        model._packed = None
        for run in runs.values():                   # the packed operands belong to the mode: drop the last mode's before building this one's
            run["lora"]._packed = None
            run["ms"], run["peak"] = [], 0.0
        torch.cuda.empty_cache()
        for r in ranks:
            for _ in range(args.warmup):
                step(runs[r])
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for r in ranks:
                run = runs[r]
                torch.cuda.reset_peak_memory_stats(dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(run)
                torch.cuda.synchronize()
                run["ms"].append(1000.0 * (time.perf_counter() - t0) / args.steps)
                run["peak"] = max(run["peak"], torch.cuda.max_memory_allocated(dev) / 1e9)
        res = {}
        for r in ranks:
            run = runs[r]
            assert bool(torch.isfinite(run["loss"])), (mode, r)
            res[name(r)] = {"layout": run["layout"], "ext_qkv_proj": run["ext"], "trainable_params": run["params"], "ms_per_step_median": statistics.median(run["ms"]),
                           "ms_per_step_rounds": run["ms"], "spread_ms": max(run["ms"]) - min(run["ms"]), "peak_hbm_gb": round(run["peak"], 1),
                           "loss_last": float(run["loss"])}
        ref = res[name(ranks[0])]["ms_per_step_median"]
        first = f"rank_{ranks[0][1]}" if not keyed else name(ranks[0])
        for r in ranks:
            res[name(r)][f"delta_vs_{first}_ms"] = res[name(r)]["ms_per_step_median"] - ref
            res[name(r)][f"delta_vs_{first}_pct"] = 100.0 * (res[name(r)]["ms_per_step_median"] - ref) / ref
        if pd > 0:                                  # the layout switch and dropout, each against its own baseline
            for k in ranks:
                if k[2] == "p0":
                    n0, nw, nd_ = res[name(k)], res[name(k[:2] + ("p0-wide",))], res[name(k[:2] + (f"p{pd:g}",))]
                    m0, mw, md = (x["ms_per_step_median"] for x in (n0, nw, nd_))
                    nw["layout_switch_vs_p0_ms"], nw["layout_switch_vs_p0_pct"] = mw - m0, 100.0 * (mw - m0) / m0
                    nd_["dropout_delta_vs_p0_wide_ms"], nd_["dropout_delta_vs_p0_wide_pct"] = md - mw, 100.0 * (md - mw) / mw
                    nd_["dropout_delta_beyond_spread"] = abs(md - mw) > max(nw["spread_ms"], nd_["spread_ms"])
        out[mode] = res
    print(json.dumps({"workload": f"HunyuanVideo-T2V denoiser ({nd} + {ns} blocks), latents 16x{lT}x{lH}x{lW}, {lT * (lH // 2) * (lW // 2)} image + "
                                  f"{Lt} text tokens, micro-batch {B}, LoRA target sets {tsets}, HunyuanVideoFlow.training_step + AdamW",
                      "rounds": args.rounds, "steps_per_block": args.steps, "warmup": args.warmup,
                      **({"lora_dropout": pd} if pd > 0 else {}), "modes": out}), flush=True)


if __name__ == "__main__":
    main()
