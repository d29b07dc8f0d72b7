"""Fixed cost per generation of the 256x256 GEMM kernel (tile mode 2, default K-loop) for the library that VT355_LIB names (default: the
in-tree one).  Times the CogVideoX block shapes at M = 71104 and derives, from the two pairs with one N at two K, the time per K-tile
and the rest per generation of the persistent grid (epilogue + tile boundary):  t(K) = gens * (nk * per_ktile + fixed).
Built for epilogue ablations: a library whose epilogue was cut gives wrong results here on purpose, nothing is compared.
usage: [VT355_LIB=lib.so] python tools/kbench_gemm_epilogue.py [--rounds 5] [--label NAME] [--out FILE (appended)]"""
import argparse, os, statistics, sys, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from vt355 import ops

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--label", default=os.environ.get("VT355_LIB", "in-tree library"))
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
BF = torch.bfloat16
CM, CS, CST = 71104, 17776, 226
SHAPES = [(CM, 1920, 1984, "bias"), (CM, 1920, 7680, "bias"), (CM, 1984, 1920, "bias"), (CM, 1984, 5760, "bias"),
          (CM, 7680, 1920, "bias"), (CM, 7680, 1920, "dgelu"), (CM, 7680, 1920, "gelu"), (CM, 1920, 7680, "gated")]


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


cus = torch.cuda.get_device_properties(0).multi_processor_count
slots = cus // 8 * 8
say(f"== {args.label}: {torch.cuda.get_device_name(0)}, {slots} slots; {args.rounds} rounds x 20 launches, shapes interleaved inside a round; us = median (max - min)")
work = []
for M, N, K, epi in SHAPES:
    a, w, c = uni(M, K), uni(N, K), torch.empty(M, N, device=dev, dtype=BF)
    kw = {}
    if epi == "dgelu":
        kw = dict(epilogue=ops.EPI_DGELU, pre_act_in=uni(M, N))
    elif epi == "gelu":
        kw = dict(epilogue=ops.EPI_BIAS_GELU, pre_act_out=torch.empty(M, N, device=dev, dtype=BF))
    elif epi == "gated":
        tab = torch.rand(M // CS, 2 * N, device=dev) + 0.5
        kw = dict(epilogue=ops.EPI_GATED_RES, residual=uni(M, N), gate_txt=tab[:, :N], gate_vid=tab[:, N:], gate_bstride=2 * N, S=CS, St=CST)
    bias = uni(N) if epi in ("bias", "gated", "gelu") else None
    work.append((a, w, c, bias, kw))
t = [[] for _ in SHAPES]
ops.gemm_set_tile(2); ops.gemm_set_big_loop(0)
try:
    for a, w, c, bias, kw in work:
        for _ in range(3):
            ops.gemm(a, w, c, bias, **kw)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for i, (a, w, c, bias, kw) in enumerate(work):
            t[i].append(timed(lambda: ops.gemm(a, w, c, bias, **kw)))
finally:
    ops.gemm_set_tile(0)
med = {}
for (M, N, K, epi), v in zip(SHAPES, t):
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    gens = -(-tiles // slots)
    med[(N, K, epi)] = (statistics.median(v), gens)
    say(f"M={M:6d} N={N:5d} K={K:5d} {epi:5s} {statistics.median(v):8.1f} us ({max(v) - min(v):5.1f})  {tiles} tiles = {gens} generations, "
        f"{statistics.median(v) / gens:6.1f} us per generation")
for N, k0, k1 in ((1920, 1984, 7680), (1984, 1920, 5760)):
    (t0, g), (t1, _) = med[(N, k0, "bias")], med[(N, k1, "bias")]
    per_kt = (t1 - t0) / g / ((k1 - k0) // 64)
    say(f"N={N}: {per_kt:.3f} us per K-tile, fixed {t0 / g - per_kt * (k0 // 64):.1f} us per generation")
(tb, g), (td, _), (tg, _) = med[(7680, 1920, "bias")], med[(7680, 1920, "dgelu")], med[(7680, 1920, "gelu")]
say(f"N=7680 K=1920: dgelu {(td - tb) / g:+.1f}, gelu + second output {(tg - tb) / g:+.1f} us per generation over bias")
(tb, g), (tg, _) = med[(1920, 7680, "bias")], med[(1920, 7680, "gated")]
say(f"N=1920 K=7680: gated {(tg - tb) / g:+.1f} us per generation over bias")
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
