"""The two K-loops of the 256x256 GEMM kernel side by side: vt_gemm_set_big_loop(1) = two-phase, (2) = eight-phase, interleaved in one
process on one card.  Per shape: ROUNDS rounds, each timing 20 launches of every arm in turn; operands are uniform random in [-1, 1).
Reports the median over the rounds and max - min, the default choice of vt_gemm_set_big_loop(0) (timed as a third arm), and -- for
pick_tile in gemm_bf16.hip -- the other two kernels (tile modes 3 and 1) and the default dispatch in the same rounds.
--block-only: the CogVideoX block rows alone (an A/B of two builds: run it once per build, VT355_LIB names the other one).
usage: python tools/kbench_gemm_big8.py [--rounds 5] [--block-only] [--out FILE]"""
import argparse, os, statistics, sys, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from vt355 import ops

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--block-only", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
BF = torch.bfloat16
CM, CS, CST = 71104, 17776, 226
# the eight block Linears of the CogVideoX-2B LoRA step at micro-batch 4 (forward: qkv, out, ff1, ff2; input gradients: out^T, qkv^T, ff2^T
# with dGELU, ... ) as the issue lists them, and ff1 as the step runs it, with GELU and the pre-activation as second output: (M, N, K, epilogue)
BENCH = [(CM, 5760, 1984, "bias"), (CM, 1920, 1984, "bias"), (CM, 7680, 1920, "bias"), (CM, 1920, 7680, "bias"), (CM, 1984, 1920, "bias"),
         (CM, 1984, 5760, "bias"), (CM, 7680, 1920, "dgelu"), (CM, 1920, 7680, "gated"), (CM, 7680, 1920, "gelu")]
# every shape of tools/kbench_gemm_shapes.py, the remaining bf16 rows of tests/test_gemm_production_gpu.py's table, two cubes and K = 64 ... 576 at N = 5120 and 640
OTHERS = [(163840, 320, 320), (40960, 640, 640), (10240, 1280, 1280), (40960, 5120, 640), (40960, 640, 2560), (163840, 2560, 320), (163840, 320, 1280),
          (10240, 10240, 1280), (10240, 1280, 5120), (16384, 1152, 1152), (16384, 3840, 1152), (16384, 4608, 1152), (16384, 1152, 4608), (16384, 1152, 1280),
          (35552, 1920, 1920), (35552, 7680, 1920), (35552, 1920, 7680), (35552, 5760, 1984), (35552, 1984, 5760),
          (142208, 5760, 1984), (142208, 7680, 1920), (142208, 1984, 5760),
          (10456, 9216, 3072), (10456, 3072, 3072), (10456, 12288, 3072), (10456, 3072, 12288), (10456, 3072, 15360), (10456, 21504, 3072),
          (71104, 64, 5760), (35552, 12288, 3072), (35552, 3072, 12288), (10200, 9216, 3136), (10200, 3072, 3136), (10200, 12288, 3072),
          (10200, 3072, 12288), (16384, 1152, 64), (452, 4096, 10240),
          (8192, 8192, 8192), (4096, 4096, 4096), (40960, 5120, 64), (40960, 5120, 128), (40960, 5120, 192), (40960, 5120, 320),
          (40960, 5120, 384), (40960, 5120, 512), (40960, 5120, 576), (40960, 640, 384), (40960, 640, 512), (40960, 640, 576)]


def uni(*shape):
    return (torch.rand(*shape, device=dev) * 2.0 - 1.0).to(BF)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / 20


lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


say(f"{torch.cuda.get_device_name(0)}; {args.rounds} rounds x 20 launches per arm, arms interleaved inside a round; us = median (max - min)")
for M, N, K, epi in BENCH + ([] if args.block_only else [(m, n, k, "bias") for m, n, k in OTHERS]):
    ops.gemm_set_tile(0)
    dflt = ops.gemm_kernel(M, N, K)
    a, w, c = uni(M, K), uni(N, K), torch.empty(M, N, device=dev, dtype=BF)
    kw = {}
    if epi == "dgelu":
        kw = dict(epilogue=ops.EPI_DGELU, pre_act_in=uni(M, N))
    elif epi == "gated":
        tab = torch.rand(M // CS, 2 * N, device=dev) + 0.5
        kw = dict(epilogue=ops.EPI_GATED_RES, residual=uni(M, N), gate_txt=tab[:, :N], gate_vid=tab[:, N:], gate_bstride=2 * N, S=CS, St=CST)
    elif epi == "gelu":
        kw = dict(epilogue=ops.EPI_BIAS_GELU, pre_act_out=torch.empty(M, N, device=dev, dtype=BF))
    bias = uni(N) if epi in ("bias", "gated", "gelu") else None
    arms = {"two-phase": (2, 1), "eight-phase": (2, 2), "default loop": (2, 0), "producer / consumer (tile 3)": (3, 0), "128x128 (tile 1)": (1, 0),
            f"default dispatch (kernel {dflt})": (0, 0)}
    t = {k: [] for k in arms}
    try:
        for k, (tile, loop) in arms.items():          # warm-up
            ops.gemm_set_tile(tile); ops.gemm_set_big_loop(loop)
            for _ in range(3):
                ops.gemm(a, w, c, bias, **kw)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for k, (tile, loop) in arms.items():
                ops.gemm_set_tile(tile); ops.gemm_set_big_loop(loop)
                t[k].append(timed(lambda: ops.gemm(a, w, c, bias, **kw)))
    finally:
        ops.gemm_set_tile(0); ops.gemm_set_big_loop(0)
    say(f"M={M:6d} N={N:5d} K={K:5d} {epi:5s} (nk {K // 64}, default dispatch: kernel {dflt})")
    for k, v in t.items():
        med = statistics.median(v)
        say(f"    {k:30s} {med:8.1f} us ({max(v) - min(v):5.1f})  {2.0 * M * N * K / med / 1e6:6.0f} TF/s")
    m1, m2 = statistics.median(t["two-phase"]), statistics.median(t["eight-phase"])
    spread = max(max(t["two-phase"]) - min(t["two-phase"]), max(t["eight-phase"]) - min(t["eight-phase"]))
    verdict = "eight-phase" if m1 - m2 > spread else "two-phase" if m2 - m1 > spread else "tie"
    say(f"    -> {verdict} ({(m1 / m2 - 1.0) * 100.0:+.1f} %)")
    del a, w, c, kw
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
