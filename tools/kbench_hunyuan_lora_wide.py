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

``--ff``: instead, the kernels of the feed-forward LoRA targets (ff.net.0.proj, ff.net.2, proj_mlp, proj_out) at M = 10 456:
  * the rank-side products at K in {3072, 12288, 15360} (the widths of x, of gelu(u) and of the single block's [attn | gelu(mlp)]) and
    ranks 4 and 64: the rank gradient dA += dt^T x (vt_lora_tn_wide, which also makes dB over the output width) and the bf16 GEMM
    with N = ext that makes t = x A^T and dt = g (scaling B), next to vt_lora_down_wide, which the attention sites use for t at K = 3072
    and these sites do not (its one block per 64 rows walks all of K: half the GEMM's rate).  Each is compared with the same kernel at K = 3072 scaled by the bytes
    it reads (K / 3072): "x bytes" above 1 means the kernel lost rate at the wide K;
  * the extended products with GELU (fc1, N 12288, K 3072 + Kt), dGELU (d u of fc2, N 12288, K 3072 + Kt) and gated-residual
    (fc2, N 3072, K 12288 + Kt; linear2, K 15360 + Kt) epilogues at tail widths Kt = 0 / 64 / 192, bf16 (one GEMM over K + Kt) and fp8
    (the bf16 tail), against the same product with Kt = 0 plus the MFMA work the tail adds: Kt / K in bf16, 2 Kt / K in fp8.

    python tools/kbench_hunyuan_lora_wide.py --ff [--rounds 20] > profiles/hunyuan_lora_ff_kbench.txt

``--drop P``: instead, the origin-map (_at) dropped rank-side kernels of lora_dropout = P at M = 10 456 (a single block's rows of one
rank of a two-rank sequence-parallel run: 5 100 image + 256 text rows ... the map is not the identity) and K in {3072, 12288, 15360},
ranks 4 and 64, one adapter (the feed-forward sites) and, at K = 3072, three (the fused q | k | v projection): each _at kernel is
launched right after its undropped sibling -- down, tn (dA), up_add, and the dgelu form of up_add against the undropped up_add.

    python tools/kbench_hunyuan_lora_wide.py --drop 0.1 [--rounds 20] > profiles/hunyuan_lora_dropout_kbench.txt
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
    ap.add_argument("--ff", action="store_true", help="the feed-forward targets' kernels instead of the attention sites' tails")
    ap.add_argument("--drop", type=float, default=0.0, help="p > 0: the dropped _at rank-side kernels next to their undropped siblings")
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
    if args.ff:
        return ff_kernels(args, torch, ops, dev)
    if args.drop > 0:
        return drop_kernels(args, torch, ops, dev)
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


def _alternate(torch, variants, warmup, rounds):
    """{key: (median, max - min)} in microseconds, every variant launched once per round"""
    times = {k: [] for k in variants}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for rd in range(warmup + rounds):
        for k, fn in variants.items():
            ev[0].record(); fn(); ev[1].record()
            ev[1].synchronize()
            if rd >= warmup:
                times[k].append(1000.0 * ev[0].elapsed_time(ev[1]))
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in times.items()}


def ff_kernels(args, torch, ops, dev):
    from vt355.ops import EPI_BIAS_GELU, EPI_DGELU, EPI_GATED_RES
    BF, M = torch.bfloat16, args.M
    gen = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, device=dev, generator=gen) * sc)
    KS = (3072, 12288, 15360)
    # ---- rank-side products
    x = rnd(M, KS[-1]).to(BF)
    variants = {}
    for r in (4, 64):
        rp = (r + 15) // 16 * 16
        a = rnd(r, KS[-1], sc=0.02).to(BF)
        t = torch.empty(M, 64, dtype=BF, device=dev)
        dt = rnd(M, 64).to(BF)
        sbt = rnd(64, KS[-1], sc=0.02).to(BF)
        for K in KS:
            gA = torch.zeros(r, K, device=dev)
            variants[("down  t = x A^T", r, K)] = lambda a=a, r=r, rp=rp, K=K, t=t: ops.lora_down_wide(x[:, :K], a[:, :K], 1, r, rp, 64, t, K)
            variants[("tn    dA += dt^T x", r, K)] = lambda r=r, K=K, gA=gA, dt=dt: ops.lora_tn_wide(x[:, :K], dt, r, gA, 1, K, 1.0, K)
            variants[("gemm  N = ext", r, K)] = lambda K=K, sbt=sbt, t=t: ops.gemm(x[:, :K], sbt[:, :K], t, None)
    res = _alternate(torch, variants, args.warmup, args.rounds)
    print("\n## rank-side products (one adapter, ext 64): microseconds median / spread, GB/s of the [M, K] operand, time over the K = 3072 time x K / 3072")
    print(f"{'kernel':>20} | {'r':>3} | " + " | ".join(f"{'K ' + str(K):>30}" for K in KS))
    for kern in ("down  t = x A^T", "tn    dA += dt^T x", "gemm  N = ext"):
        for r in (4, 64):
            base = res[(kern, r, 3072)][0]
            cells = []
            for K in KS:
                med, spr = res[(kern, r, K)]
                cells.append(f"{med:8.1f} / {spr:5.1f} {2.0 * M * K / med / 1e3:6.0f} GB/s x{med / (base * K / 3072):5.2f}")
            print(f"{kern:>20} | {r:>3} | " + " | ".join(f"{c:>30}" for c in cells))
    del x, variants
    # ---- extended products
    print("\n## extended products: microseconds median / spread; cost of the tail over Kt = 0 against the MFMA work it adds")
    KTS = (0, 64, 192)
    for label, N, K, epi in (("fc1 / linear1 MLP rows, GELU", 12288, 3072, "gelu"), ("d u of fc2 / linear2, dGELU", 12288, 3072, "dgelu"),
                             ("fc2, gated residual", 3072, 12288, "gated"), ("linear2, gated residual", 3072, 15360, "gated")):
        xe, we = rnd(M, K + 192).to(BF), rnd(N, K + 192, sc=K ** -0.5).to(BF)
        aq, sa = ops.quantize_fp8(xe[:, :K].contiguous())
        wq, sw = ops.quantize_fp8(we[:, :K].contiguous())
        gq = aq.float().to(torch.float8_e5m2)
        bias = rnd(N, sc=0.1).to(BF)
        y, u = torch.empty(M, N, dtype=BF, device=dev), rnd(M, N).to(BF)
        gate = rnd(1, N).float()
        if epi == "gelu":
            kb = dict(epilogue=EPI_BIAS_GELU, pre_act_out=u); kq = kb
        elif epi == "dgelu":
            kb = dict(epilogue=EPI_DGELU, pre_act_in=u); kq = kb
        else:
            kb = dict(epilogue=EPI_GATED_RES, residual=u, gate_txt=gate, gate_vid=gate, gate_bstride=N, S=M, St=0); kq = kb
        variants = {}
        for Kt in KTS:
            tail = dict(tail=(xe[:, K:K + Kt], we[:, K:K + Kt])) if Kt else {}
            variants[("bf16", Kt)] = lambda Kt=Kt: ops.gemm(xe[:, :K + Kt], we[:, :K + Kt], y, None if epi == "dgelu" else bias, **kb)
            if epi == "dgelu":
                variants[("fp8", Kt)] = lambda tail=tail: ops.gemm_mxfp8_dx(gq, wq, y, sa, sw, **kq, **tail)
            else:
                variants[("fp8", Kt)] = lambda tail=tail: ops.gemm_mxfp8(aq, wq, y, sa, sw, bias, **kq, **tail)
        res = _alternate(torch, variants, args.warmup, args.rounds)
        print(f"\n### {label}: N {N}, K {K}")
        print(f"{'Kt':>4} | {'bf16 K + Kt':>16} | {'over Kt 0':>14} | {'added work':>10} | {'fp8 + bf16 tail':>16} | {'over Kt 0':>14} | {'added work':>10}")
        for Kt in KTS:
            (bm, bs), (qm, qs) = res[("bf16", Kt)], res[("fp8", Kt)]
            ob, oq = bm - res[("bf16", 0)][0], qm - res[("fp8", 0)][0]
            print(f"{Kt:>4} | {bm:8.1f} / {bs:5.1f} | {ob:7.1f} {100 * ob / res[('bf16', 0)][0]:5.1f}% | {100.0 * Kt / K:9.1f}% | "
                  f"{qm:8.1f} / {qs:5.1f} | {oq:7.1f} {100 * oq / res[('fp8', 0)][0]:5.1f}% | {200.0 * Kt / K:9.1f}%")
        del xe, we, aq, wq, gq, y, u, variants


def drop_kernels(args, torch, ops, dev):
    BF, M, p, seed = torch.bfloat16, args.M, args.drop, 20230211
    gen = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, device=dev, generator=gen) * sc)
    KS = (3072, 12288, 15360)
    Lt = 256
    Lil = M - Lt                                            # rank 1 of 2: its image rows start at Lil, the text rows sit behind 2 Lil
    og = lambda K: (M, 2 * Lil + Lt, Lil, Lil, Lil, 0, K)
    x, u = rnd(M, KS[-1]).to(BF), rnd(M, KS[-1]).to(BF)
    dx = rnd(M, KS[-1]).to(BF)
    variants, order = {}, []
    for r in (4, 64):
        rp = (r + 15) // 16 * 16
        for n, K in [(1, K) for K in KS] + [(3, 3072)]:
            ext = (n * rp + 63) // 64 * 64
            a = rnd(n * r, K, sc=0.02).to(BF)
            t = torch.empty(M, ext, dtype=BF, device=dev)
            dt = rnd(M, ext, sc=0.1).to(BF)
            gA = torch.zeros(r, K, device=dev)
            key = lambda kern, kind, r=r, n=n, K=K: (kern, r, n, K, kind)
            order.append((r, n, K))
            variants[key("down", "plain")] = lambda a=a, n=n, r=r, rp=rp, ext=ext, t=t, K=K: ops.lora_down_wide(x[:, :K], a, n, r, rp, ext, t, K)
            variants[key("down", "drop")] = lambda a=a, n=n, r=r, rp=rp, ext=ext, t=t, K=K: [
                ops.lora_down_wide_drop_at(x[:, :K], a[j * r:], g, r, rp, ext - j * rp if j + g == n else g * rp, t[:, j * rp:], K, p, seed, j, og(K))
                for j, g in _groups(ops, n, rp)]
            variants[key("tn", "plain")] = lambda r=r, K=K, gA=gA, dt=dt: ops.lora_tn_wide(x[:, :K], dt, r, gA, 1, K, 1.0, K)
            variants[key("tn", "drop")] = lambda r=r, K=K, gA=gA, dt=dt: ops.lora_tn_wide_drop_at(x[:, :K], dt, r, gA, 1, K, 1.0, K, p, seed, 0, og(K))
            variants[key("up_add", "plain")] = lambda a=a, n=n, r=r, rp=rp, dt=dt, K=K: ops.lora_up_add_wide(dx[:, :K], dt, a, n, r, rp, K)
            variants[key("up_add", "drop")] = lambda a=a, n=n, r=r, rp=rp, dt=dt, K=K: ops.lora_up_add_wide_drop_at(dx[:, :K], dt, a, n, r, rp, K, p, seed, 0, og(K))
            variants[key("up_add", "dgelu")] = lambda a=a, n=n, r=r, rp=rp, dt=dt, K=K: ops.lora_up_add_wide_dgelu_drop_at(
                dx[:, :K], dt, a, n, r, rp, u[:, :K], K, p, seed, 0, og(K))
    res = _alternate(torch, variants, args.warmup, args.rounds)
    print(f"\n## lora_dropout {p}: each _at kernel right after its undropped sibling; microseconds median / spread, ratio to the sibling")
    print("## tn is one adapter per call at any n; down at n = 3, r = 64 is two calls (2 + 1 adapters: the masked x blocks of three do not fit the LDS)")
    print(f"{'kernel':>8} | {'r':>3} | {'n':>1} | {'K':>5} | {'undropped':>16} | {'_drop_at':>16} | {'ratio':>5} | {'dgelu _drop_at':>16} | {'ratio':>5}")
    for kern in ("down", "tn", "up_add"):
        for r, n, K in order:
            (pm, ps), (dm, ds) = res[(kern, r, n, K, "plain")], res[(kern, r, n, K, "drop")]
            g = res.get((kern, r, n, K, "dgelu"))
            gcell = f"{g[0]:8.1f} / {g[1]:5.1f} | {g[0] / pm:5.2f}" if g else f"{'-':>16} | {'-':>5}"
            print(f"{kern:>8} | {r:>3} | {n:>1} | {K:>5} | {pm:8.1f} / {ps:5.1f} | {dm:8.1f} / {ds:5.1f} | {dm / pm:5.2f} | {gcell}")


def _groups(ops, n, rp):
    """(first adapter, adapters) of each vt_lora_down_wide_drop_at call for n adapters: the engine's grouping (_HYRun.drop_down)"""
    out, j = [], 0
    while j < n:
        g = n - j
        while g > 1 and not ops.lora_down_wide_drop_fits(g, rp):
            g -= 1
        out.append((j, g))
        j += g
    return out


if __name__ == "__main__":
    main()
