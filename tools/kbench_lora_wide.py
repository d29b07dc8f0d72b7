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

--drop P (> 0) times the lora_dropout sibling of every kernel that has one right after it ("path" ends in "+drop"; tn_dB reads the saved
T and has none): same bytes, plus one Philox4x32-10 per 4 elements and adapter.  "vs_sibling" is its median over the sibling's.  Above
rank 80 three masked X blocks do not fit the LDS and the dropped down-projection is three calls, one per adapter.

    python tools/kbench_lora_wide.py [--launches 20] [--warmup 5] > profiles/lora_wide_kbench.txt
    python tools/kbench_lora_wide.py --drop 0.1 --ranks 4,16,32,64,128 > profiles/lora_dropout_kbench.txt
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUSTAINED_GBPS = 5607.6          # profiles/gradclip_kbench.txt, vt_adamw at 1.41 G elements
SUSTAINED_TFLOPS = 1090.0        # DESIGN 5, gemm_*_bf16 in the step


def ff_section(args, ops, torch, dev, M, d, g, line, last, P, SEED):
    """--ff: the single-adapter products of the feed-forward LoRA targets (ff.net.0.proj reads K = d, ff.net.2 reads K = 4 d), each rank in
    the layout the engine picks for it (narrow up to 16, wide above): the three rank-side products at K = 4 d next to K = d, the dgelu_drop
    form of the dX correction right after its _drop sibling ("vs_sibling": time ratio; its bytes add the read of U), and the W2^T product
    with the dGELU epilogue at K = d + ext (the undropped correction folded in) against K = d.

        python tools/kbench_lora_wide.py --ff --ranks 4,64 > profiles/lora_ff_kbench.txt"""
    from vt355.lora import extension_layout
    from vt355.ops import EPI_DGELU
    BF = torch.bfloat16
    for r in [int(v) for v in args.ranks.split(",")]:
        rp, _, ext, wide = extension_layout(r)
        path = "wide" if wide else "narrow"
        for K in (d, 4 * d):
            tag = f"K={K}"
            x = torch.randn(M, K + ext, device=dev, generator=g).to(BF)
            A = (torch.randn(r, K, device=dev, generator=g) * 0.02).to(BF)
            gA, gB = torch.zeros(r, K, device=dev), torch.zeros(K, r, device=dev)
            t = x[:, K:]
            if wide:
                down = lambda: ops.lora_down_wide(x, A, 1, r, rp, ext, t, K)
                dB = lambda: ops.lora_tn_wide(x, t, r, gB, r, 1, 0.25, K)
                dA = lambda: ops.lora_tn_wide(x, t, r, gA, 1, K, 1.0, K)
                up = lambda: ops.lora_up_add_wide(x, t, A, 1, r, rp, K)
                up_drop = lambda: ops.lora_up_add_wide_drop(x, t, A, 1, r, rp, K, P, SEED, 0)
            else:
                down = lambda: ops.lora_down(x, A, r, t, K)
                dB = lambda: ops.skinny_tn(x, t, r, gB, r, 1, 0.25, K)
                dA = lambda: ops.skinny_tn(x, t, r, gA, 1, K, 1.0, K)
                up = lambda: ops.lora_up_add(x, t, A, r, K)
                up_drop = lambda: ops.lora_up_add_drop(x, t, A, r, 1, K, P, SEED, 0)
            tn_bytes, flops = 2.0 * (M * K + M * r) + 8.0 * K * r, 2.0 * M * K * r
            up_bytes = 2.0 * (2 * M * K + M * rp + r * K)
            line("down", r, f"{path} {tag}", down, 2.0 * (M * K + r * K + M * ext), flops)
            line("tn_dB", r, f"{path} {tag}", dB, tn_bytes, flops)
            line("tn_dA", r, f"{path} {tag}", dA, tn_bytes, flops)
            t.mul_(0.01)                      # the in-place correction is repeated: keep the sum finite
            line("up_add", r, f"{path} {tag}", up, up_bytes, flops)
            args.drop = P
            line("up_add", r, f"{path} {tag}+drop", up_drop, up_bytes, flops)
            if K == 4 * d:                    # ff.net.2: the correction enters before the dGELU
                u = torch.randn(M, K, device=dev, generator=g).to(BF)
                if wide:
                    fn = lambda: ops.lora_up_add_wide_dgelu_drop(x, t, A, 1, r, rp, u, K, P, SEED, 0)
                else:
                    fn = lambda: ops.lora_up_add_dgelu_drop(x, t, A, r, 1, u, K, P, SEED, 0)
                rec = line("up_add", r, f"{path} {tag} dgelu_drop", fn, up_bytes + 2.0 * M * K, flops)
                print(json.dumps({"kernel": "up_add", "rank": r, "path": f"{path} {tag} dgelu_drop", "lora_dropout": P,
                                  "vs_drop_sibling": round(rec["median_ms"] / last[("up_add", f"{path} {tag}+drop")], 3)}), flush=True)
                del u
            del x, A, gA, gB, t
        # the W2^T product with the dGELU epilogue: [tg | dT2] [W2^T | A2^T]^T at K = d + ext against tg W2 at K = d
        tgx = torch.randn(M, d + ext, device=dev, generator=g).to(BF)
        w2t = (torch.randn(4 * d, d + ext, device=dev, generator=g) * 0.02).to(BF)
        u = torch.randn(M, 4 * d, device=dev, generator=g).to(BF)
        du = torch.empty(M, 4 * d, dtype=BF, device=dev)
        for K in (d, d + ext):
            line("gemm_dgelu_w2t", r, f"K={K}", lambda: ops.gemm(tgx, w2t, du, None, epilogue=EPI_DGELU, pre_act_in=u, K=K),
                 2.0 * (M * K + 4 * d * K + 2 * M * 4 * d), 2.0 * M * 4 * d * K)
        del tgx, w2t, u, du
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=35552)
    ap.add_argument("--dim", type=int, default=1920)
    ap.add_argument("--drop", type=float, default=0.0, help="P > 0: also time the lora_dropout siblings")
    ap.add_argument("--ranks", default="16,32,64,128", help="ranks <= 16 also run the narrow kernels")
    ap.add_argument("--ff", action="store_true", help="the feed-forward targets' shapes instead (ff_section below)")
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

    SEED, last = 0x2F3C5A7E9B1D4C68 >> 2, {}

    def line(kernel, r, path, fn, nbytes, flops, launches_per_call=1):
        med, spread = timed(fn)
        rec = {"kernel": kernel, "rank": r, "path": path, "rows": M, "dim": d, "launches_per_call": launches_per_call,
               "median_ms": round(med, 4), "spread_ms": round(spread, 4), "timed_launches": args.launches,
               "algorithmic_mb": round(nbytes / 1e6, 1), "algorithmic_gflop": round(flops / 1e9, 2),
               "gb_per_s": round(nbytes / 1e9 / (med / 1e3), 1), "tflop_per_s": round(flops / 1e12 / (med / 1e3), 2),
               "frac_of_sustained_hbm": round(nbytes / 1e9 / (med / 1e3) / SUSTAINED_GBPS, 3),
               "frac_of_sustained_mfma": round(flops / 1e12 / (med / 1e3) / SUSTAINED_TFLOPS, 4)}
        if path.endswith("+drop"):
            rec["lora_dropout"] = args.drop
            rec["vs_sibling"] = round(med / last[(kernel, path[:-5])], 3)
        last[(kernel, path)] = med
        print(json.dumps(rec), flush=True)
        return rec

    print(json.dumps({"sustained_gb_per_s": SUSTAINED_GBPS, "sustained_gb_per_s_source": "profiles/gradclip_kbench.txt (vt_adamw, 1.41 G elements)",
                      "sustained_tflop_per_s": SUSTAINED_TFLOPS, "sustained_tflop_per_s_source": "DESIGN 5: gemm_*_bf16 in the training step",
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    P = args.drop
    if args.ff:
        return ff_section(args, ops, torch, dev, M, d, g, line, last, P if P > 0 else 0.1, SEED)
    for r in [int(v) for v in args.ranks.split(",")]:
        force = r <= 16
        rp, eq, eo, _ = extension_layout(r, wide=True)
        x1 = torch.randn(M, d + eq, device=dev, generator=g).to(BF)
        dy = torch.randn(M, d, device=dev, generator=g).to(BF)
        A = (torch.randn(3 * r, d, device=dev, generator=g) * 0.02).to(BF)
        gB = torch.zeros(d, r, device=dev)
        gA = torch.zeros(r, d, device=dev)
        path = "wide (forced)" if force else "wide"
        line("down", r, path, lambda: ops.lora_down_wide(x1, A, 3, r, rp, eq, x1[:, d:], d),
             2.0 * (M * d + 3 * r * d + M * eq), 2.0 * M * d * 3 * r)
        if P > 0:
            one = ops.lora_down_wide_drop_fits(3, rp)

            def down_drop():
                if one:
                    ops.lora_down_wide_drop(x1, A, 3, r, rp, eq, x1[:, d:], d, P, SEED, 0)
                else:
                    for j in range(3):
                        ops.lora_down_wide_drop(x1, A[j * r:(j + 1) * r], 1, r, rp, rp if j < 2 else eq - 2 * rp, x1[:, d + j * rp:], d, P, SEED, j)
            line("down", r, path + "+drop", down_drop, 2.0 * ((1 if one else 3) * M * d + 3 * r * d + M * eq), 2.0 * M * d * 3 * r, 1 if one else 3)
        line("tn_dB", r, path, lambda: ops.lora_tn_wide(dy, x1[:, d:], r, gB, r, 1, 0.25, d),
             2.0 * (M * d + M * r) + 8.0 * d * r, 2.0 * M * d * r)
        line("tn_dA", r, path, lambda: ops.lora_tn_wide(x1, x1[:, d:], r, gA, 1, d, 1.0, d),
             2.0 * (M * d + M * r) + 8.0 * d * r, 2.0 * M * d * r)
        if P > 0:
            line("tn_dA", r, path + "+drop", lambda: ops.lora_tn_wide_drop(x1, x1[:, d:], r, gA, 1, d, 1.0, d, P, SEED, 0),
                 2.0 * (M * d + M * r) + 8.0 * d * r, 2.0 * M * d * r)
        x1[:, d:].mul_(0.01)                  # the in-place correction is repeated: keep the sum finite
        line("up_add", r, path, lambda: ops.lora_up_add_wide(x1, x1[:, d:], A, 3, r, rp, d),
             2.0 * (2 * M * d + M * 3 * rp + 3 * r * d), 2.0 * M * d * 3 * r)
        if P > 0:
            line("up_add", r, path + "+drop", lambda: ops.lora_up_add_wide_drop(x1, x1[:, d:], A, 3, r, rp, d, P, SEED, 0),
                 2.0 * (2 * M * d + M * 3 * rp + 3 * r * d), 2.0 * M * d * 3 * r)
        if r <= 16:                           # the narrow kernels at the same rank, as the engine issues them: one call up to 3 r = 16, else one per adapter
            xn = torch.randn(M, d + 64, device=dev, generator=g).to(BF)
            nc = 1 if 3 * r <= 16 else 3                       # calls per projection
            Rc, na = (3 * r, 3) if nc == 1 else (r, 1)         # rank columns and adapters per call

            def down_narrow():
                if nc == 1:
                    return ops.lora_down(xn, A, 3 * r, xn[:, d:], d)
                for j in range(3):
                    ops.lora_down(xn, A[j * r:(j + 1) * r], r, xn[:, d + j * r:], d, zero_cols=(64 - 2 * r - 16) if j == 2 else 0)

            def down_narrow_drop():
                if nc == 1:
                    return ops.lora_down_drop(xn, A, 3 * r, 3, xn[:, d:], d, P, SEED, 0)
                for j in range(3):
                    ops.lora_down_drop(xn, A[j * r:(j + 1) * r], r, 1, xn[:, d + j * r:], d, P, SEED, j, zero_cols=(64 - 2 * r - 16) if j == 2 else 0)

            def up_narrow():
                for j in range(nc):
                    ops.lora_up_add(xn, xn[:, d + j * r:], A[j * r:j * r + Rc], Rc, d)

            def up_narrow_drop():
                for j in range(nc):
                    ops.lora_up_add_drop(xn, xn[:, d + j * r:], A[j * r:j * r + Rc], Rc, na, d, P, SEED, j)

            gAn = torch.zeros(Rc, d, device=dev)
            line("down", r, "narrow", down_narrow, 2.0 * (nc * M * d + 3 * r * d + M * 64), 2.0 * M * d * 3 * r, nc)
            if P > 0:
                line("down", r, "narrow+drop", down_narrow_drop, 2.0 * (nc * M * d + 3 * r * d + M * 64), 2.0 * M * d * 3 * r, nc)
            line("tn_dB", r, "narrow", lambda: ops.skinny_tn(dy, xn[:, d:], r, gB, r, 1, 0.25, d), 2.0 * (M * d + M * r) + 8.0 * d * r, 2.0 * M * d * r)
            line("tn_dA", r, "narrow", lambda: ops.skinny_tn(xn, xn[:, d:], Rc, gAn, 1, d, 1.0, d), 2.0 * (M * d + M * Rc) + 8.0 * d * Rc, 2.0 * M * d * Rc)
            if P > 0:
                line("tn_dA", r, "narrow+drop", lambda: ops.skinny_tn_drop(xn, xn[:, d:], Rc, na, gAn, 1, d, 1.0, d, P, SEED, 0),
                     2.0 * (M * d + M * Rc) + 8.0 * d * Rc, 2.0 * M * d * Rc)
            xn[:, d:].mul_(0.01)
            line("up_add", r, "narrow", up_narrow, 2.0 * (nc * 2 * M * d + M * 3 * r + 3 * r * d), 2.0 * M * d * 3 * r, nc)
            if P > 0:
                line("up_add", r, "narrow+drop", up_narrow_drop, 2.0 * (nc * 2 * M * d + M * 3 * r + 3 * r * d), 2.0 * M * d * 3 * r, nc)
            del xn
        del x1, dy
    return 0


if __name__ == "__main__":
    sys.exit(main())
