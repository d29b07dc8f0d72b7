#!/usr/bin/env python3
"""Kernel bench of the CogVideoX VAE decoder's two kernels at every level's real shape (latent 13 x 60 x 90 -> 49 x 480 x 720), the
materialised alternative of the fused upsample in the same run, and the whole decode with its peak HBM.

One process; for every shape the candidates are launched ALTERNATELY, 20 timed launches each after a warm-up of every shape, device
events around each launch; the figures are the median and the spread (max - min) of the 20.  Needs a GPU: there is no fallback.

  vt_upsample_conv2d_cl      fused: the nearest-upsampled tensor is never stored
  materialised               F.interpolate(nearest) written to memory (channels-last), then the per-frame 3x3 convolution (vt_conv_cl); both
                             per group of frames (vt_conv_cl addresses at most 2 GiB of input per call, torch's upsample 2^31 elements)
  vt_spatialnorm_silu_cl     statistics + finalize + gathering apply (the modulation table is given; its GEMM is timed on its own line)

Usage: python tools/kbench_vae_decoder.py [--out profiles/vae_decoder_kbench.txt] [--launches 20]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vt355 import ops  # noqa: E402
from vt355.vae import CogVideoXVaeDecoder  # noqa: E402

BF16 = torch.bfloat16
LAT = (13, 60, 90)
# (C, T, H, W, temporal) of the three Upsample3D of the CogVideoX decoder, in the order it runs them
UP_SHAPES = ((512, 13, 60, 90, True), (256, 25, 120, 180, True), (256, 49, 240, 360, False))
# (C, T, H, W) of every distinct SpatialNorm3D shape
SPN_SHAPES = ((512, 13, 60, 90), (512, 25, 120, 180), (256, 25, 120, 180), (256, 49, 240, 360), (256, 49, 480, 720), (128, 49, 480, 720))
PEAK_BF16, PEAK_HBM = 2516.6e12, 8.0e12           # spec: dense bf16 MFMA FLOP/s, HBM3E bytes/s


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return statistics.median(ms), max(ms) - min(ms)


def rand(shape, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty(shape, dtype=BF16, device=dev)
    flat = out.view(-1)
    step = 1 << 28
    for i in range(0, flat.numel(), step):
        flat[i:i + step] = torch.randn(min(step, flat.numel() - i), generator=g, device=dev).to(BF16)
    return out


def bench_upsample(C, T, H, W, tup, n, dev, log):
    x = rand((1, T, H, W, C), dev, 1)
    w = (torch.randn(C, C, 3, 3, device=dev) / (9 * C) ** 0.5).to(BF16)
    wk, b = ops.pack_conv_weight(w), torch.zeros(C, dtype=BF16, device=dev)
    ts = ops.upsample_src_frames(T, tup)
    To = len(ts)
    y1 = torch.empty(1, To, 2 * H, 2 * W, C, dtype=BF16, device=dev)
    y2 = torch.empty_like(y1)
    tsd = torch.tensor(ts, device=dev)
    group = max(1, (3 << 29) // (4 * H * W * C * 2))               # frames per vt_conv_cl call: at most 1.5 GiB of input

    def fused():
        ops.upsample_conv2d(x, wk, b, y1, tup)

    def materialised():
        src = x[0].index_select(0, tsd) if tup and T > 1 else x[0]                        # [To, H, W, C]
        for t0 in range(0, To, group):                                                    # per group: torch's upsample indexes in 32 bits
            u = F.interpolate(src[t0:t0 + group].permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")      # channels-last memory, written
            u = u.permute(0, 2, 3, 1)                                                     # [group, 2H, 2W, C]
            assert u.is_contiguous()
            ops.conv_cl(u.unsqueeze(0), wk, y2[0, t0:t0 + group].unsqueeze(0), (1, 3, 3), (0, 1, 1), bias=b)

    fused(); materialised()
    torch.cuda.synchronize()
    same = bool(torch.equal(y1, y2))
    diff = (y1.view(-1)[:1 << 24].float() - y2.view(-1)[:1 << 24].float()).abs().max().item()
    tf, tm = [], []
    for _ in range(n):
        tf.append(timed(fused)); tm.append(timed(materialised))
    flop = 2.0 * To * 4 * H * W * C * C * 9
    (mf, sf), (mm, sm) = stats(tf), stats(tm)
    log(f"upsample C={C} {T}x{H}x{W} -> {To}x{2 * H}x{2 * W} temporal={int(tup)}  ({flop / 1e12:.2f} TFLOP, output {y1.numel() * 2 / 1e9:.2f} GB)")
    log(f"    fused vt_upsample_conv2d_cl   median {mf:8.3f} ms  spread {sf:6.3f} ms  {flop / mf / 1e9:7.1f} TFLOP/s  {100 * flop / PEAK_BF16 / (mf / 1e3):5.1f} % of the MFMA bound")
    log(f"    materialised upsample + conv  median {mm:8.3f} ms  spread {sm:6.3f} ms  {flop / mm / 1e9:7.1f} TFLOP/s")
    log(f"    outputs bit-identical: {same} (max |diff| over the first 2^24 elements {diff:.3g});  fused ahead by {mm - mf:.3f} ms, larger spread {max(sf, sm):.3f} ms")
    return mf, sf, mm, sm


def bench_spn(C, T, H, W, n, dev, log):
    Tz, Hz, Wz = LAT
    x = rand((1, T, H, W, C), dev, 2)
    y = torch.empty_like(x)
    zq = torch.zeros(1, Tz, Hz, Wz, 64, dtype=BF16, device=dev)
    zq[..., :16] = torch.randn(1, Tz, Hz, Wz, 16, device=dev).to(BF16)
    wm = (torch.randn(2 * C, 64, device=dev) / 4).to(BF16)
    bm = torch.zeros(2 * C, dtype=BF16, device=dev)
    mod = torch.empty(1, Tz, Hz, Wz, 2 * C, dtype=BF16, device=dev)
    gamma, beta = torch.ones(C, dtype=BF16, device=dev), torch.zeros(C, dtype=BF16, device=dev)
    ws = torch.empty(4 * C, dtype=torch.float32, device=dev)

    def table():
        ops.gemm(zq.view(-1, 64), wm, mod.view(-1, 2 * C), bm)

    def spn():
        ops.spatialnorm_silu(x, gamma, beta, mod, y, 32, 1e-6, True, ws)

    table(); spn()
    torch.cuda.synchronize()
    tt, tsn = [], []
    for _ in range(n):
        tt.append(timed(table)); tsn.append(timed(spn))
    nbytes = 3.0 * x.numel() * 2                                   # x read by the statistics pass and by the apply pass, y written
    (mt, st), (ms_, ss) = stats(tt), stats(tsn)
    log(f"spatialnorm C={C} {T}x{H}x{W}  ({x.numel() * 2 / 1e9:.2f} GB)   median {ms_:8.3f} ms  spread {ss:6.3f} ms  {nbytes / ms_ / 1e9:6.2f} TB/s of 3 passes  "
        f"{100 * nbytes / PEAK_HBM / (ms_ / 1e3):5.1f} % of the HBM bound;  table GEMM median {mt:.3f} ms  spread {st:.3f} ms")
    return ms_


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_decoder_kbench.txt"))
    ap.add_argument("--launches", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_vae_decoder needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"# tools/kbench_vae_decoder.py on {torch.cuda.get_device_name(0)}: median and spread (max - min) of {a.launches} alternating launches per candidate")
    ups = [bench_upsample(*s, a.launches, dev, log) for s in UP_SHAPES]
    torch.cuda.empty_cache()
    ahead = [mm - mf > max(sf, sm) for (mf, sf, mm, sm) in ups[-2:]]
    log(f"decision (last two levels, fused median below materialised by more than the larger spread): {ahead} -> "
        f"{'the fused kernel ships' if all(ahead) else 'the materialised path ships'}")
    spn_ms = {s: bench_spn(*s, a.launches, dev, log) for s in SPN_SHAPES}
    torch.cuda.empty_cache()

    # ---- whole decode of a 13 x 60 x 90 latent, peak HBM
    m = CogVideoXVaeDecoder().init_weights(1).to(dev)
    z = torch.randn(1, 16, *LAT, generator=torch.Generator().manual_seed(6))
    m(z); torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t = [timed(lambda: m(z)) for _ in range(5)]
    peak = torch.cuda.max_memory_allocated()
    md, sd = stats(t)
    log(f"whole decode 13x60x90 -> 49x480x720: median {md:.1f} ms  spread {sd:.1f} ms of 5;  peak HBM {peak / 1e9:.2f} GB allocated "
        f"({base / 1e9:.2f} GB of it weights and packed copies)")
    # per decode: SpatialNorm3D count per shape (2 per block, norm_out) and the three upsamples
    counts = {(512, 13, 60, 90): 12, (512, 25, 120, 180): 1, (256, 25, 120, 180): 7, (256, 49, 240, 360): 8, (256, 49, 480, 720): 1,
              (128, 49, 480, 720): 7 + 1}
    spn_total = sum(spn_ms[s] * c for s, c in counts.items())
    up_total = sum(u[0] for u in ups)
    log(f"of the decode: vt_spatialnorm_silu_cl {spn_total:.1f} ms ({100 * spn_total / md:.1f} %), vt_upsample_conv2d_cl {up_total:.1f} ms ({100 * up_total / md:.1f} %) "
        f"(kernel medians above x launches per decode)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
