"""The wide bf16 tail of vt_gemm_mxfp8 / vt_gemm_mxfp8_dx at HunyuanVideo's adapted Linears (M = 10 456 rows, K = 3072, N = 9216: the
fused q | k | v projection, N = 3072: img_attn_proj) against what the kernels without it can do for the same product:
  tail  the fp8 product with the K-extension as its bf16 tail (Kt = 0: no tail; 64: the straight-from-global tail; 192, 384: LDS-staged)
  (a)   the fp8 product without a tail, then the bf16 correction y += t (sB)^T as ops.gemm(t, sB, y, epilogue=EPI_GATED_RES, residual=y)
  (b)   the plain bf16 ops.gemm over K = D + Kt
forward (bias epilogue) and input-gradient product (vt_gemm_mxfp8_dx, "+ residual" epilogue, E5M2 gradient).  Every variant of a shape is
launched once per round for --rounds rounds in one process (alternating, HIP-event times); the table gives the median and the spread
(max - min) in microseconds, the cost of the tail over Kt = 0 and, next to it, the MFMA work the tail adds: Kt bf16 columns count as
2 Kt fp8 columns at the instruction rates, i.e. 2 Kt / K of the fp8 product.

    python tools/kbench_hunyuan_lora_wide.py [--rounds 20] > profiles/hunyuan_lora_wide_kbench.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--M", type=int, default=10456)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from vt355 import ops
    from vt355.ops import EPI_GATED_RES
    if not torch.cuda.is_available():
        raise SystemExit("kbench_hunyuan_lora_wide needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    BF, M, K = torch.bfloat16, args.M, 3072
    gen = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, device=dev, generator=gen) * sc)
    print(f"# M {M}, K {K}; median / spread (max - min) over {args.rounds} alternating launches, microseconds")
    for N in (9216, 3072):
        aq, sa = ops.quantize_fp8(rnd(M, K).to(BF))
        wq, sw = ops.quantize_fp8(rnd(N, K, sc=K ** -0.5).to(BF))
        gq = aq.float().to(torch.float8_e5m2)
        bias = rnd(N, sc=0.1).to(BF)
        res = rnd(M, N).to(BF)
        xe, we = rnd(M, K + 384).to(BF), rnd(N, K + 384, sc=K ** -0.5).to(BF)       # the extended bf16 operands: [x | t], [W | sB]
        y = torch.empty(M, N, dtype=BF, device=dev)
        variants = {}
        for Kt in (0, 64, 192, 384):
            t, sB = xe[:, K:K + Kt], we[:, K:K + Kt]
            tail = dict(tail=(t, sB)) if Kt else {}
            variants[("fwd", "tail", Kt)] = lambda tail=tail: ops.gemm_mxfp8(aq, wq, y, sa, sw, bias, **tail)
            variants[("dx", "tail", Kt)] = lambda tail=tail: ops.gemm_mxfp8_dx(gq, wq, y, sa, sw, epilogue=EPI_GATED_RES, residual=res, **tail)
            if Kt:
                def comp_fwd(t=t, sB=sB):
                    ops.gemm_mxfp8(aq, wq, y, sa, sw, bias)
                    ops.gemm(t, sB, y, None, epilogue=EPI_GATED_RES, residual=y)

                def comp_dx(t=t, sB=sB):
                    ops.gemm_mxfp8_dx(gq, wq, y, sa, sw, epilogue=EPI_GATED_RES, residual=res)
                    ops.gemm(t, sB, y, None, epilogue=EPI_GATED_RES, residual=y)
                variants[("fwd", "(a)", Kt)] = comp_fwd
                variants[("dx", "(a)", Kt)] = comp_dx
            variants[("fwd", "(b)", Kt)] = lambda Kt=Kt: ops.gemm(xe[:, :K + Kt], we[:, :K + Kt], y, bias)
            variants[("dx", "(b)", Kt)] = lambda Kt=Kt: ops.gemm(xe[:, :K + Kt], we[:, :K + Kt], y, None, epilogue=EPI_GATED_RES, residual=res)
        times = {k: [] for k in variants}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for rd in range(args.warmup + args.rounds):
            for k, fn in variants.items():
                ev[0].record(); fn(); ev[1].record()
                ev[1].synchronize()
                if rd >= args.warmup:
                    times[k].append(1000.0 * ev[0].elapsed_time(ev[1]))
        med = {k: statistics.median(v) for k, v in times.items()}
        spr = {k: max(v) - min(v) for k, v in times.items()}
        for kind in ("fwd", "dx"):
            print(f"\n## N {N}, {'forward, bias epilogue' if kind == 'fwd' else 'vt_gemm_mxfp8_dx, + residual, e5m2 gradient'}")
            print(f"{'Kt':>4} | {'tail':>16} | {'(a) fp8 + bf16 fix':>18} | {'(b) bf16 K+Kt':>16} | {'tail - Kt0':>14} | {'added MFMA work':>15} | verdict")
            for Kt in (0, 64, 192, 384):
                f = lambda k: f"{med[k]:8.1f} / {spr[k]:5.1f}"
                tl, a, b = (kind, "tail", Kt), (kind, "(a)", Kt), (kind, "(b)", Kt)
                over = med[tl] - med[(kind, "tail", 0)]
                verdict = ""
                if Kt:
                    bar = max(spr[tl], spr[a], spr[b])
                    verdict = "beats both" if (med[a] - med[tl] > bar and med[b] - med[tl] > bar) else "DOES NOT beat both by more than the spread"
                print(f"{Kt:>4} | {f(tl):>16} | {(f(a) if Kt else '-'):>18} | {f(b):>16} | {over:7.1f} {100 * over / med[(kind, 'tail', 0)]:5.1f}% | "
                      f"{100.0 * 2 * Kt / K:14.1f}% | {verdict}")
        del aq, wq, gq, res, xe, we, y


if __name__ == "__main__":
    main()
