"""vt_gemm_mxfp8 (MX-scaled fp8, v_mfma_scale_f32_16x16x128_f8f6f4) vs vt_gemm_fp8 (non-scaled fp8 MFMA) vs the bf16 GEMM (ops.gemm) on
HunyuanVideo's block shapes: the five of profiles/r02_fp8_gemm_kbench.txt plus the single blocks' linear1 (N 21504, K 3072) and linear2
(N 3072, K 15360) at 10 240 rows.  Random operands, device-event timing after a warm-up, the mean of `--iters` launches.  Each line: ms,
TFLOP/s (2 M N K over the time) and the fraction of the dense peak of the kernel's input type (fp8 ~5 PF, bf16 ~2.5 PF) and of the fp8
peak; the last column checks that the MX-fp8 and the non-scaled fp8 kernels compute the same product (rel-L2 of their outputs)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_mxfp8 needs the GPU")
    dev = torch.device("cuda:0")
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
