"""vt_gemm_mxfp8 (MX-scaled fp8, v_mfma_scale_f32_16x16x128_f8f6f4) vs vt_gemm_fp8 (non-scaled fp8 MFMA) vs the bf16 GEMM (ops.gemm) on
HunyuanVideo's block shapes: the five of profiles/r02_fp8_gemm_kbench.txt plus the single blocks' linear1 (N 21504, K 3072) and linear2
(N 3072, K 15360) at 10 240 rows.  Random operands, device-event timing after a warm-up, the mean of `--iters` launches.  Each line: ms,
TFLOP/s (2 M N K over the time) and the fraction of the dense peak of the kernel's input type (fp8 ~5 PF, bf16 ~2.5 PF) and of the fp8
peak; the last column checks that the MX-fp8 and the non-scaled fp8 kernels compute the same product (rel-L2 of their outputs).

``--dx``: the input-gradient products of fp8_dgrad instead, at the bench workload's 10 456 rows: vt_gemm_bf16 (against a bf16 transposed
weight, today's backward) vs vt_gemm_mxfp8_dx with the gradient in E5M2 and in E4M3 -- qkv, proj, fc1, fc2 (dGELU, with the fp8 copy of
d(u)), and linear1 / linear2 split as the model splits them (column / row slices of the transposed weight, "+ residual", the dGELU columns
written into the joint d(cat) buffer) -- then vt_gate_mul vs vt_gate_mul_fp8 on a [10 456, 3072] gradient.

``--amax``: the kernels that publish an amax (vt_cast_fp8_scaled, vt_gate_mul_fp8, vt_ln_modulate_fwd_fp8, vt_quantize_fp8, the GELU
epilogue of vt_gemm_mxfp8 with its fp8 copy) at 10 456 rows, every launch against a cleared slot as in a training step.  Run it once
with the shipped library and once with VT355_LIB pointing at a build with -DVT_AMAX_ALWAYS_ATOMIC (csrc/build.sh with VT_EXTRA_FLAGS,
VT_OBJ_DIR, VT_LIB_NAME) for the A/B of the read-before-atomic publisher (csrc/common.h: amax_publish)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from vt355 import ops  # noqa: E402

PEAK_FP8, PEAK_BF16 = 5.0e15, 2.5e15
SHAPES = [(10240, 9216, 3072), (10240, 3072, 3072), (10240, 12288, 3072), (10240, 3072, 12288), (32768, 9216, 3072),
          (10240, 21504, 3072), (10240, 3072, 15360)]


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters / 1e3


def dx_bench(dev, iters):
    from vt355.ops import EPI_DGELU, EPI_GATED_RES
    BF = torch.bfloat16
    M, D, M4 = 10456, 3072, 12288
    g = torch.Generator(device=dev).manual_seed(0)
    one = torch.ones(1, device=dev)

    def operands(N, K, wt_shape=None, r0=0, c0=0):
        """gradient [M, K] in bf16 / E5M2 / E4M3 and the [N, K] slice (at row r0, column c0) of a transposed weight of shape wt_shape"""
        R, C = wt_shape or (N, K)
        gb = torch.randn(M, K, device=dev, generator=g).to(BF)
        wt = (torch.randn(R, C, device=dev, generator=g) * K ** -0.5).to(BF)
        wq, sw = ops.quantize_fp8(wt)
        amax = gb.float().abs().max()
        gq = {}
        for dt, fmax in ((ops.FP8_E5M2, 57344.0), (ops.FP8, 448.0)):
            q = torch.empty(M, K, dtype=dt, device=dev)
            sc = (amax / fmax).reshape(1)
            ops.cast_fp8_fmt(gb, q, sc, torch.zeros(1, device=dev))
            gq[dt] = (q, sc)
        return gb, wt[r0:r0 + N, c0:c0 + K], wq[r0:r0 + N, c0:c0 + K], sw, gq

    cases = [("qkv", D, 3 * D, None, 0, 0, "plain"), ("proj", D, D, None, 0, 0, "plain"), ("fc1", D, M4, None, 0, 0, "plain"),
             ("fc2", M4, D, None, 0, 0, "dgelu"),
             ("linear1[qkv rows]", D, 3 * D, (D, 3 * D + M4), 0, 0, "plain"), ("linear1[mlp rows]", D, M4, (D, 3 * D + M4), 0, 3 * D, "res"),
             ("linear2[attn cols]", D, D, (D + M4, D), 0, 0, "plain"), ("linear2[mlp cols]", M4, D, (D + M4, D), D, 0, "dgelu")]
    for name, N, K, wts, r0, c0, epi in cases:
        gb, wt, wq, sw, gq = operands(N, K, wts, r0, c0)
        wide = name.startswith("linear2")                   # both products of linear2 write column ranges of one [M, D + M4] buffer
        buf = torch.empty(M, D + M4 if wide else N, dtype=BF, device=dev)
        out = buf[:, D:] if name == "linear2[mlp cols]" else buf[:, :N]
        u = torch.randn(M, N, device=dev, generator=g).to(BF) if epi == "dgelu" else None
        res = torch.randn(M, N, device=dev, generator=g).to(BF) if epi == "res" else None
        kb = dict(epilogue=EPI_DGELU, pre_act_in=u) if epi == "dgelu" else dict(epilogue=EPI_GATED_RES, residual=res) if epi == "res" else {}
        tb = timed(lambda: ops.gemm(gb, wt, out, None, **kb), iters)
        ref = out.double().clone()
        ts, rels = {}, {}
        for dt, (q, sc) in gq.items():
            kq = dict(kb)
            if epi == "dgelu":                               # the fp8 copy of d(u) rides along, as in the model
                kq["out_fp8"] = (torch.empty(M, N, dtype=dt, device=dev), one, torch.zeros(1, device=dev))
            ts[dt] = timed(lambda: ops.gemm_mxfp8_dx(q, wq, out, sc, sw, **kq), iters)
            rels[dt] = ((out.double() - ref).norm() / ref.norm()).item()
        fl = 2.0 * M * N * K
        t5, t4 = ts[ops.FP8_E5M2], ts[ops.FP8]
        print(f"dX {name} ({epi}) M {M} N {N} K {K}: bf16 {tb * 1e3:.3f} ms = {fl / tb / 1e12:.0f} TFLOP/s | mxfp8_dx e5m2 {t5 * 1e3:.3f} ms = "
              f"{fl / t5 / 1e12:.0f} TFLOP/s ({tb / t5:.2f}x) | e4m3 {t4 * 1e3:.3f} ms = {fl / t4 / 1e12:.0f} TFLOP/s ({tb / t4:.2f}x) | "
              f"output vs bf16 product rel-L2 e5m2 {rels[ops.FP8_E5M2]:.1e} e4m3 {rels[ops.FP8]:.1e}", flush=True)
        del gb, wt, wq, gq, buf, out, u, res, ref
    x = torch.randn(M, D, device=dev, generator=g).to(BF)
    gate = torch.randn(1, 6 * D, device=dev, generator=g)[:, :D]
    y = torch.empty(M, D, dtype=BF, device=dev)
    tg = timed(lambda: ops.gate_mul(x, y, gate, gate, 6 * D, D, M, 0), iters)
    row = [f"gate_mul [{M}, {D}]: bf16 only {tg * 1e6:.1f} us"]
    for dt, nm in ((ops.FP8_E5M2, "e5m2"), (ops.FP8, "e4m3")):
        q = torch.empty(M, D, dtype=dt, device=dev)
        am = torch.zeros(1, device=dev)
        tz = timed(lambda: am.zero_(), iters)            # the slot is cleared once a step: time every launch against an empty slot
        tq = timed(lambda: (am.zero_(), ops.gate_mul_fp8(x, y, gate, gate, 6 * D, D, M, 0, q, one, am)), iters) - tz
        tc = timed(lambda: (am.zero_(), ops.cast_fp8_fmt(y, q, one, am)), iters) - tz
        row.append(f"gate_mul_fp8 {nm} {tq * 1e6:.1f} us (+{(tq - tg) * 1e6:.1f}); a separate cast pass {tc * 1e6:.1f} us")
    print(" | ".join(row), flush=True)


def amax_bench(dev, iters):
    from vt355._lib import lib_path
    from vt355.ops import EPI_BIAS_GELU
    BF = torch.bfloat16
    M, D, M4 = 10456, 3072, 12288
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(M, D, device=dev, generator=g).to(BF)
    y = torch.empty(M, D, dtype=BF, device=dev)
    q = torch.empty(M, D, dtype=ops.FP8, device=dev)
    one = torch.ones(1, device=dev)
    am = torch.zeros(1, device=dev)
    gate = torch.randn(1, 6 * D, device=dev, generator=g)
    sh, sc = gate[:, :D], gate[:, D:2 * D]
    mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
    w = (torch.randn(M4, D, device=dev, generator=g) * D ** -0.5).to(BF)
    wq, sw = ops.quantize_fp8(w)
    xq, sx = ops.quantize_fp8(x)
    o4, u4 = torch.empty(M, M4, dtype=BF, device=dev), torch.empty(M, M4, dtype=BF, device=dev)
    q4 = torch.empty(M, M4, dtype=ops.FP8, device=dev)
    tz = timed(lambda: am.zero_(), iters)
    cases = [("vt_cast_fp8_scaled [10456, 3072]", lambda: ops.cast_fp8_scaled(x, q, one, am)),
             ("vt_gate_mul_fp8 [10456, 3072]", lambda: ops.gate_mul_fp8(x, y, sh, sh, 6 * D, D, M, 0, q, one, am)),
             ("vt_ln_modulate_fwd_fp8 [10456, 3072]", lambda: ops.ln_modulate_fwd_fp8(x, y, None, None, (sh, sc, sh, sc, 6 * D), mean, rstd, D, M, 0,
                                                                                       1e-6, q, one, am)),
             ("vt_gemm_mxfp8 GELU + fp8 copy M 10456 N 12288 K 3072", lambda: ops.gemm_mxfp8(xq, wq, o4, sx, sw, None, epilogue=EPI_BIAS_GELU,
                                                                                               pre_act_out=u4, out_fp8=(q4, one, am)))]
    print(f"library {os.path.basename(lib_path())}", flush=True)
    for name, fn in cases:
        t = timed(lambda: (am.zero_(), fn()), iters) - tz
        print(f"  {name}: {t * 1e6:.1f} us", flush=True)
    t = timed(lambda: ops.quantize_fp8(x), iters)           # clears its own slot
    print(f"  vt_quantize_fp8 [10456, 3072] (amax pass + scale + cast): {t * 1e6:.1f} us", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dx", action="store_true", help="the fp8_dgrad input-gradient products and the fused gate multiply")
    ap.add_argument("--amax", action="store_true", help="the amax-publishing kernels against a cleared slot (A/B through VT355_LIB)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_mxfp8 needs the GPU")
    dev = torch.device("cuda:0")
    if args.amax:
        amax_bench(dev, args.iters)
        return
    if args.dx:
        dx_bench(dev, args.iters)
        return
    BF = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    for (M, N, K) in SHAPES:
        a = torch.randn(M, K, device=dev, generator=g).to(BF)
        w = (torch.randn(N, K, device=dev, generator=g) * K ** -0.5).to(BF)
        aq, sa = ops.quantize_fp8(a)
        wq, sw = ops.quantize_fp8(w)
        o8 = torch.empty(M, N, dtype=BF, device=dev)
        omx = torch.empty(M, N, dtype=BF, device=dev)
        ob = torch.empty(M, N, dtype=BF, device=dev)
        tb = timed(lambda: ops.gemm(a, w, ob), args.iters)
        t8 = timed(lambda: ops.gemm_fp8(aq, wq, o8, sa, sw), args.iters)
        tm = timed(lambda: ops.gemm_mxfp8(aq, wq, omx, sa, sw), args.iters)
        rel = ((omx.double() - o8.double()).norm() / o8.double().norm()).item()
        fl = 2.0 * M * N * K
        row = " | ".join(f"{n} {t * 1e3:.3f} ms = {fl / t / 1e12:.0f} TFLOP/s ({fl / t / pk:.3f} of {pkn} peak{'' if pkn == 'fp8' else f', {fl / t / PEAK_FP8:.3f} of fp8'})"
                         for n, t, pk, pkn in (("bf16", tb, PEAK_BF16, "bf16"), ("fp8", t8, PEAK_FP8, "fp8"), ("mxfp8", tm, PEAK_FP8, "fp8")))
        print(f"M {M} N {N} K {K}: {row} | mxfp8 / fp8 {t8 / tm:.2f}x, / bf16 {tb / tm:.2f}x | mxfp8 vs fp8 output rel-L2 {rel:.1e}", flush=True)
        del a, w, aq, wq, o8, omx, ob


if __name__ == "__main__":
    main()
