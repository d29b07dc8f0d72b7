"""The wide (rank 17..128) LoRA rank-side kernels of csrc/lora_wide.hip alone, at the CogVideoX-2B shapes of two 17 776-token samples:
M = 35 552 rows, d = 1920, ranks 16 (wide layout forced), 32, 64, 128.  Per kernel: HIP-event time per launch (median and spread of
--launches launches after warm-up, every launch timed on its own), the bytes the algorithm must move and its FLOPs computed from the
shapes, and both as a fraction of what the box sustains.  For rank 16 the narrow kernels (csrc/lora.hip) are timed in the same run.

  down      qkv down-projection, three adapters in one pass: reads X [M, d] (and A, 3 r x d), writes T [M, ext]
  tn_dB     dB of one adapter: Big = dY [M, d] slice, Small = T_j [M, r]            -> out [d, r]   (osr == 1)
  tn_dA     dA of one adapter: Big = x [M, d],       Small = dT_j [M, r]           -> out [r, d]   (osp == 1)
  up_add    dX correction, three adapters at once: reads dT [M, 3 rp] and dX [M, d], writes dX [M, d]

Sustained rates: the HBM figure is the one profiles/gradclip_kbench.txt measured with a streaming kernel on this kind of box (vt_adamw on
1.41 G elements: 5607.6 GB/s); the MFMA figure is what the library's large bf16 GEMMs hold inside the training step (1080-1100
TFLOP/s; 1090 used).  A fraction is algorithmic work over time over that rate, not a counter reading.

    python tools/kbench_lora_wide.py [--launches 20] [--warmup 5] > profiles/lora_wide_kbench.txt
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUSTAINED_GBPS = 5607.6          # profiles/gradclip_kbench.txt, vt_adamw at 1.41 G elements
SUSTAINED_TFLOPS = 1090.0        # DESIGN 5, gemm_*_bf16 in the step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=35552)
    ap.add_argument("--dim", type=int, default=1920)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from vt355 import ops
    from vt355.lora import extension_layout
    if not torch.cuda.is_available():
        raise SystemExit("kbench_lora_wide needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    BF = torch.bfloat16
    M, d = args.rows, args.dim
    g = torch.Generator(device=dev).manual_seed(5)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts), max(ts) - min(ts)

    def line(kernel, r, path, fn, nbytes, flops, launches_per_call=1):
        med, spread = timed(fn)
        rec = {"kernel": kernel, "rank": r, "path": path, "rows": M, "dim": d, "launches_per_call": launches_per_call,
               "median_ms": round(med, 4), "spread_ms": round(spread, 4), "timed_launches": args.launches,
               "algorithmic_mb": round(nbytes / 1e6, 1), "algorithmic_gflop": round(flops / 1e9, 2),
               "gb_per_s": round(nbytes / 1e9 / (med / 1e3), 1), "tflop_per_s": round(flops / 1e12 / (med / 1e3), 2),
               "frac_of_sustained_hbm": round(nbytes / 1e9 / (med / 1e3) / SUSTAINED_GBPS, 3),
               "frac_of_sustained_mfma": round(flops / 1e12 / (med / 1e3) / SUSTAINED_TFLOPS, 4)}
        print(json.dumps(rec), flush=True)
        return rec

    print(json.dumps({"sustained_gb_per_s": SUSTAINED_GBPS, "sustained_gb_per_s_source": "profiles/gradclip_kbench.txt (vt_adamw, 1.41 G elements)",
                      "sustained_tflop_per_s": SUSTAINED_TFLOPS, "sustained_tflop_per_s_source": "DESIGN 5: gemm_*_bf16 in the training step",
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    for r, force in ((16, True), (32, False), (64, False), (128, False)):
        rp, eq, eo, _ = extension_layout(r, wide=True)
        x1 = torch.randn(M, d + eq, device=dev, generator=g).to(BF)
        dy = torch.randn(M, d, device=dev, generator=g).to(BF)
        A = (torch.randn(3 * r, d, device=dev, generator=g) * 0.02).to(BF)
        gB = torch.zeros(d, r, device=dev)
        gA = torch.zeros(r, d, device=dev)
        path = "wide (forced)" if force else "wide"
        line("down", r, path, lambda: ops.lora_down_wide(x1, A, 3, r, rp, eq, x1[:, d:], d),
             2.0 * (M * d + 3 * r * d + M * eq), 2.0 * M * d * 3 * r)
        line("tn_dB", r, path, lambda: ops.lora_tn_wide(dy, x1[:, d:], r, gB, r, 1, 0.25, d),
             2.0 * (M * d + M * r) + 8.0 * d * r, 2.0 * M * d * r)
        line("tn_dA", r, path, lambda: ops.lora_tn_wide(x1, x1[:, d:], r, gA, 1, d, 1.0, d),
             2.0 * (M * d + M * r) + 8.0 * d * r, 2.0 * M * d * r)
        x1[:, d:].mul_(0.01)                  # the in-place correction is repeated: keep the sum finite
        line("up_add", r, path, lambda: ops.lora_up_add_wide(x1, x1[:, d:], A, 3, r, rp, d),
             2.0 * (2 * M * d + M * 3 * rp + 3 * r * d), 2.0 * M * d * 3 * r)
        if r == 16:                           # the narrow kernels at the same rank: one call per adapter, as the engine issues them
            xn = torch.randn(M, d + 64, device=dev, generator=g).to(BF)

            def down_narrow():
                for j in range(3):
                    ops.lora_down(xn, A[j * r:(j + 1) * r], r, xn[:, d + j * r:], d, zero_cols=(64 - 2 * r - 16) if j == 2 else 0)

            def up_narrow():
                for j in range(3):
                    ops.lora_up_add(xn, xn[:, d + j * r:], A[j * r:(j + 1) * r], r, d)

            line("down", r, "narrow", down_narrow, 2.0 * (3 * M * d + 3 * r * d + M * 64), 2.0 * M * d * 3 * r, 3)
            line("tn_dB", r, "narrow", lambda: ops.skinny_tn(dy, xn[:, d:], r, gB, r, 1, 0.25, d), 2.0 * (M * d + M * r) + 8.0 * d * r, 2.0 * M * d * r)
            line("tn_dA", r, "narrow", lambda: ops.skinny_tn(xn, xn[:, d:], r, gA, 1, d, 1.0, d), 2.0 * (M * d + M * r) + 8.0 * d * r, 2.0 * M * d * r)
            xn[:, d:].mul_(0.01)
            line("up_add", r, "narrow", up_narrow, 2.0 * (3 * 2 * M * d + M * 3 * r + 3 * r * d), 2.0 * M * d * 3 * r, 3)
            del xn
        del x1, dy
    return 0


if __name__ == "__main__":
    sys.exit(main())
