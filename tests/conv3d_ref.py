"""fp64 references, an exact input family and the case list for the VAE's implicit-GEMM convolutions (csrc/conv3d.hip:
conv3d_cl_kernel, 128-row tiles; conv3d_pc_kernel, 256-row tiles, persistent, loader / multiplier waves; the 8-channel first convolution).

  * causal_conv3d_ref / downsample_conv2d_ref: the formula at the top of conv3d.hip restated with explicit loops over the 27 / 9 taps on
    padded tensors -- first frame replicated twice in front of t and zeros around h / w; one zero line / column at the bottom / right and
    stride 2.  No F.conv3d / F.conv2d here: tests/test_conv3d_cpu.py pins these loops to them, so the two stay independent.
    `displace` moves ONE tap's read by (dt, dh, dw) positions: the wrong convolution the CPU test uses to show that the inputs discriminate.
  * exact_inputs: x integers in [-2, 2], weights in {-1, 0, 1}, bias multiples of 4 up to 128, residual multiples of 8 up to 512 (all exact
    in bf16).  Every partial sum is an integer below 2^24, so fp32 accumulation is exact in any order; the epilogue adds bias and residual
    in fp32 (gemm_epilogue_apply: o = v + bias, then r + o, both exact here) and rounds ONCE, pack2's `(bf16_t)float`, which is
    round-to-nearest-even.  The device result must equal round_bf16(reference) bit for bit.  Bias and residual push many results past 256,
    where bf16 holds even integers only, so the rounding -- ties included -- is exercised, not just the sum.
  * CASES: the smallest shapes at which each thing can go wrong, with the launch plan each must get under a forced kernel, written down
    by hand from the kernels' tiling rules (not computed by a copy of the library's launch code).  tests/test_conv3d_gpu.py imports them.
  * REAL_CONVS: every convolution of the real encoder and decoder with the kernel the shape rule gives it on an MI355X.
Pure torch, no GPU: the CPU and the GPU tests draw identical tensors from a seed."""
import functools
from collections import namedtuple

import torch

BF = torch.bfloat16
LIMIT = 1 << 24


def round_bf16(t):
    """fp64 integers below 2^24 -> bf16, one round-to-nearest-even (fp64 -> fp32 is exact for them; torch's fp32 -> bf16 is RNE)"""
    return t.float().to(BF)


def _epilogue(y, bias, res):
    if bias is not None:
        y = y + bias.double()
    if res is not None:
        y = y + res.double()
    return y


def causal_conv3d_ref(x, w, bias=None, res=None, displace=None):
    """x [N,T,H,W,Cin], w [Cout,Cin,3,3,3] -> fp64 [N,T,H,W,Cout]:
    y[n,t,h,w,:] = bias + res + sum_{dt,dh,dw} W[:,:,dt,dh,dw] x[n, max(t+dt-2, 0), h+dh-1, w+dw-1, :], zero outside h / w.
    displace = ((dt, dh, dw), (et, eh, ew)): that one tap reads where tap (et, eh, ew) would (a deliberately wrong convolution)"""
    x, w = x.double(), w.double()
    N, T, H, W, Cin = x.shape
    xp = torch.zeros(N, T + 2, H + 2, W + 2, Cin, dtype=torch.float64)
    xp[:, 2:, 1:H + 1, 1:W + 1] = x
    xp[:, 0, 1:H + 1, 1:W + 1] = x[:, 0]
    xp[:, 1, 1:H + 1, 1:W + 1] = x[:, 0]
    y = torch.zeros(N * T * H * W, w.shape[0], dtype=torch.float64)
    for dt in range(3):
        for dh in range(3):
            for dw in range(3):
                et, eh, ew = displace[1] if displace is not None and displace[0] == (dt, dh, dw) else (dt, dh, dw)
                y += xp[:, et:et + T, eh:eh + H, ew:ew + W].reshape(-1, Cin) @ w[:, :, dt, dh, dw].t()
    return _epilogue(y.view(N, T, H, W, -1), bias, res)


def downsample_conv2d_ref(x, w, bias=None, res=None, displace=None):
    """x [N,T,H,W,Cin] (H, W even), w [Cout,Cin,3,3] -> fp64 [N,T,H/2,W/2,Cout]:
    y[n,t,ho,wo,:] = bias + res + sum_{dh,dw} W[:,:,dh,dw] x[n, t, 2 ho + dh, 2 wo + dw, :], zero at line H and column W.
    displace = ((dh, dw), (eh, ew)) as in causal_conv3d_ref; the padded tensor has two spare lines / columns for it"""
    x, w = x.double(), w.double()
    N, T, H, W, Cin = x.shape
    Ho, Wo = H // 2, W // 2
    xp = torch.zeros(N, T, H + 2, W + 2, Cin, dtype=torch.float64)
    xp[:, :, :H, :W] = x
    y = torch.zeros(N * T * Ho * Wo, w.shape[0], dtype=torch.float64)
    for dh in range(3):
        for dw in range(3):
            eh, ew = displace[1] if displace is not None and displace[0] == (dh, dw) else (dh, dw)
            y += xp[:, :, eh:eh + 2 * Ho:2, ew:ew + 2 * Wo:2].reshape(-1, Cin) @ w[:, :, dh, dw].t()
    return _epilogue(y.view(N, T, Ho, Wo, -1), bias, res)


# ------------------------------------------------------------------------------------------------ cases
# op: "c3" vt_causal_conv3d_cl, "ds" vt_downsample_conv2d_cl (H, W are the INPUT's), "in8" vt_causal_conv3d_in8_cl (Cin <= 8 used channels).
# res: with a residual (EPI_GATED_RES) or without (EPI_BIAS).  slots: the persistent-grid cap given to conv3d_set_kernel for the
# producer / consumer run (0 = the device's own, 256 on an MI355X).  pads = (x, y, residual) extra elements per position: x's hold NaN, y's
# are checked bit for bit.  pc = (grid, tiles, most tiles per workgroup) of the producer / consumer launch, cl = tiles (= grid) of the
# 128-row launch; None for in8, which has one kernel.  randn: the case also runs randn inputs on both kernels.
Case = namedtuple("Case", "op N T H W Cin Cout res slots pads pc cl randn")


def _c(op, N, T, H, W, Cin, Cout, res=False, slots=0, pads=(0, 0, 0), pc=None, cl=None, randn=False):
    return Case(op, N, T, H, W, Cin, Cout, res, slots, pads, pc, cl, randn)


# 256-row tiles: M = positions, nbm = ceil(M / 256), nbn = ceil(Cout / 128), tiles = nbm nbn (column tile inner: tile = 2 or 3 * row tile +
# column tile), grid = slots, or tiles rounded up to 8 when there are fewer tiles than slots; slot s walks tiles s, s + grid, ...
CASES = {
    # ---- one ragged 256-row tile: 210 positions, samples of 105 -- rows 0..104 and 105..209 have different sample and frame origins
    "straddle_64_64": _c("c3", 2, 3, 5, 7, 64, 64, pc=(8, 1, 1), cl=2, randn=True),
    "straddle_64_64_res": _c("c3", 2, 3, 5, 7, 64, 64, res=True, pc=(8, 1, 1), cl=2),
    # T = 1: every dt reads frame 0; three samples of 54 positions in one tile
    "single_frame": _c("c3", 3, 1, 6, 9, 64, 64, pc=(8, 1, 1), cl=2),
    # Wo = 3 < 4: 270 positions, a frame is 27 rows, a tile covers 9.5 frames of two samples and 85 lines
    "narrow_w3": _c("c3", 2, 5, 9, 3, 64, 64, res=True, pc=(8, 2, 1), cl=3),
    # ---- rows at exactly 256, 257 and 511
    "rows_256": _c("c3", 1, 4, 8, 8, 64, 64, pc=(8, 1, 1), cl=2),
    # 257 frames of one position: row 256 opens the second tile and reads frames 254..256, two of them behind the tile's first row
    "rows_257": _c("c3", 1, 257, 1, 1, 64, 64, res=True, pc=(8, 2, 1), cl=3),
    "rows_511": _c("c3", 1, 1, 7, 73, 64, 64, pc=(8, 2, 1), cl=4),
    # ---- column tiles: 132 = ragged second tile (4 columns), 256 = two full, 320 = three, the last half empty
    "cout_132": _c("c3", 2, 3, 5, 7, 64, 132, res=True, pc=(8, 2, 1), cl=4),
    "cout_256": _c("c3", 2, 3, 5, 7, 64, 256, pc=(8, 2, 1), cl=4),
    "cout_320": _c("c3", 2, 3, 5, 7, 64, 320, res=True, pc=(8, 3, 1), cl=6),
    # ---- two K-tiles per tap
    "cin_128": _c("c3", 2, 3, 5, 7, 128, 64, pc=(8, 1, 1), cl=2, randn=True),
    "cin_128_res": _c("c3", 2, 3, 5, 7, 128, 132, res=True, pc=(8, 2, 1), cl=4),
    # ---- grid rounding on the device's own grid: 600 positions x 320 columns = 3 x 3 = 9 tiles -> 16 workgroups, 7 of them return at once
    "grid_rounding": _c("c3", 2, 3, 10, 10, 64, 320, pc=(16, 9, 1), cl=15),
    # ---- several tiles per workgroup, slots = 8.  2432 positions x 256 columns = 10 x 2 = 20 tiles: workgroups walk 3,3,3,3,2,2,2,2
    "handover_nbn2": _c("c3", 2, 4, 16, 19, 64, 256, slots=8, pc=(8, 20, 3), cl=38, randn=True),
    "handover_nbn2_res": _c("c3", 2, 4, 16, 19, 64, 256, res=True, slots=8, pc=(8, 20, 3), cl=38, randn=True),
    # 1728 positions x 320 columns = 7 x 3 = 21 tiles: 3,3,3,3,3,2,2,2, and tile + 8 is another column tile (8 % 3 != 0); two K-tiles per tap
    "handover_nbn3": _c("c3", 2, 3, 16, 18, 128, 320, slots=8, pc=(8, 21, 3), cl=42, randn=True),
    "handover_nbn3_res": _c("c3", 2, 3, 16, 18, 128, 320, res=True, slots=8, pc=(8, 21, 3), cl=42),
    # the shipped grid: 34 560 positions x 256 columns = 135 x 2 = 270 tiles on 256 workgroups, 14 of which walk two tiles
    "device_grid": _c("c3", 1, 3, 96, 120, 64, 256, res=True, pc=(256, 270, 2), cl=540),
    # ---- the stride-2 downsample (H, W even; the zero line / column at the far edges only).  210 output positions in one tile, two samples
    "down_straddle": _c("ds", 2, 3, 10, 14, 64, 64, pc=(8, 1, 1), cl=2, randn=True),
    "down_straddle_res": _c("ds", 2, 3, 10, 14, 64, 132, res=True, pc=(8, 2, 1), cl=4),
    # 1280 output positions x 256 columns = 5 x 2 = 10 tiles on 8 workgroups: 2,2,1,1,1,1,1,1; two K-tiles per tap
    "down_handover": _c("ds", 1, 4, 32, 40, 128, 256, slots=8, pc=(8, 10, 2), cl=20, randn=True),
    "down_handover_res": _c("ds", 1, 4, 32, 40, 128, 256, res=True, slots=8, pc=(8, 10, 2), cl=20, randn=True),
    # ---- strided operands: position strides wider than the channels, NaN in x's pads, y's pads checked
    "strided": _c("c3", 2, 3, 5, 7, 64, 132, res=True, pads=(8, 4, 12), pc=(8, 2, 1), cl=4, randn=True),
    "strided_handover": _c("c3", 2, 4, 16, 19, 64, 256, res=True, slots=8, pads=(24, 8, 4), pc=(8, 20, 3), cl=38),
    "strided_down": _c("ds", 1, 4, 32, 40, 128, 256, res=True, slots=8, pads=(8, 12, 4), pc=(8, 10, 2), cl=20),
    # ---- the channel pairs that take the producer / consumer kernel in the real VAE (REAL_CONVS), forced at small sizes
    "pair_128_256": _c("c3", 2, 3, 5, 7, 128, 256, res=True, pc=(8, 2, 1), cl=4),
    "pair_256_256": _c("c3", 2, 4, 16, 19, 256, 256, res=True, slots=8, pc=(8, 20, 3), cl=38),
    "pair_512_256": _c("c3", 2, 3, 10, 10, 512, 256, pc=(8, 6, 1), cl=10),
    # ---- the 8-channel first convolution (one kernel, 8 taps per K-tile) at the same edges
    "in8_straddle": _c("in8", 2, 3, 5, 7, 3, 64),
    "in8_cout_132": _c("in8", 2, 3, 5, 7, 8, 132),
    "in8_rows_256": _c("in8", 1, 4, 8, 8, 3, 128),
    "in8_rows_257": _c("in8", 1, 257, 1, 1, 3, 64),
    "in8_rows_511": _c("in8", 1, 1, 7, 73, 3, 320),
    "in8_narrow_w3": _c("in8", 2, 5, 9, 3, 3, 64),
}
PC_CASES = tuple(n for n, c in CASES.items() if c.op != "in8")
IN8_CASES = tuple(n for n, c in CASES.items() if c.op == "in8")
RANDN_CASES = tuple(n for n, c in CASES.items() if c.randn)

# Every convolution the real models launch through vt_causal_conv3d_cl (kt 3, stride 1) / vt_downsample_conv2d_cl (kt 1, stride 2), taken
# from vt355/vae.py, one sample: the encoder on 49 x 480 x 720 (the convolutions see the whole clip; frame batches of 8 after the first 9
# only cut the GroupNorm statistics) and the decoder on a 13 x 60 x 90 latent.  (what, T, H, W of the INPUT, Cin, Cout, kt, stride, kernel):
# kernel = what vt_conv3d_plan reports with mode 0 on an MI355X (256 CUs: two or more column tiles and >= 4096 tiles of 256 x 128).
REAL_CONVS = (
    ("enc down.0 conv1/conv2 x3", 49, 480, 720, 128, 128, 3, 1, 1),
    ("enc down.0 downsample", 25, 480, 720, 128, 128, 1, 2, 1),
    ("enc down.1.block.0 conv1", 25, 240, 360, 128, 256, 3, 1, 2),
    ("enc down.1 conv 256", 25, 240, 360, 256, 256, 3, 1, 2),
    ("enc down.1 downsample", 13, 240, 360, 256, 256, 1, 2, 1),
    ("enc down.2 conv1/conv2 x3", 13, 120, 180, 256, 256, 3, 1, 1),
    ("enc down.2 downsample", 13, 120, 180, 256, 256, 1, 2, 1),
    ("enc down.3.block.0 conv1", 13, 60, 90, 256, 512, 3, 1, 1),
    ("enc down.3 / mid conv 512", 13, 60, 90, 512, 512, 3, 1, 1),
    ("enc conv_out", 13, 60, 90, 512, 32, 3, 1, 1),
    ("dec conv_in (latent padded to 64)", 13, 60, 90, 64, 512, 3, 1, 1),
    ("dec mid / up.3 conv 512", 13, 60, 90, 512, 512, 3, 1, 1),
    ("dec up.2.block.0 conv1", 25, 120, 180, 512, 256, 3, 1, 2),
    ("dec up.2 conv 256", 25, 120, 180, 256, 256, 3, 1, 2),
    ("dec up.1 conv 256", 49, 240, 360, 256, 256, 3, 1, 2),
    ("dec up.0.block.0 conv1", 49, 480, 720, 256, 128, 3, 1, 1),
    ("dec up.0 conv 128", 49, 480, 720, 128, 128, 3, 1, 1),
    ("dec conv_out (4 output rows)", 49, 480, 720, 128, 4, 3, 1, 1),
)
REAL_PC_PAIRS = {(128, 256), (256, 256), (512, 256)}


def out_hw(c):
    return (c.H // 2, c.W // 2) if c.op == "ds" else (c.H, c.W)


def positions(c):
    Ho, Wo = out_hw(c)
    return c.N * c.T * Ho * Wo


def _seed(name):
    return 1000 + list(CASES).index(name)


def _weight_shape(c):
    return (c.Cout, c.Cin, 3, 3) if c.op == "ds" else (c.Cout, c.Cin, 3, 3, 3)


@functools.lru_cache(maxsize=None)
def exact_inputs(name):
    """-> (x [N,T,H,W,Cin], w (torch layout), bias [Cout], res like y or None), fp32 holding integers exact in bf16"""
    c = CASES[name]
    g = torch.Generator().manual_seed(_seed(name))
    Ho, Wo = out_hw(c)
    x = torch.randint(-2, 3, (c.N, c.T, c.H, c.W, c.Cin), generator=g).float()
    w = torch.randint(-1, 2, _weight_shape(c), generator=g).float()
    bias = 4.0 * torch.randint(-32, 33, (c.Cout,), generator=g).float()
    res = 8.0 * torch.randint(-64, 65, (c.N, c.T, Ho, Wo, c.Cout), generator=g).float() if c.res else None
    return x, w, bias, res


@functools.lru_cache(maxsize=None)
def randn_inputs(name):
    """-> (x, w, bias, res) fp32 holding bf16 values, scaled as test_causal_conv3d_channels_last scales them"""
    c = CASES[name]
    g = torch.Generator().manual_seed(7 * _seed(name))
    Ho, Wo = out_hw(c)
    taps = 9 if c.op == "ds" else 27
    rb = lambda t: t.to(BF).float()
    x = rb(torch.randn(c.N, c.T, c.H, c.W, c.Cin, generator=g))
    w = rb(torch.randn(_weight_shape(c), generator=g) * (1.0 / (taps * c.Cin) ** 0.5))
    bias = rb(torch.randn(c.Cout, generator=g))
    res = rb(torch.randn(c.N, c.T, Ho, Wo, c.Cout, generator=g)) if c.res else None
    return x, w, bias, res


def reference_of(c, x, w, bias, res, displace=None):
    return (downsample_conv2d_ref if c.op == "ds" else causal_conv3d_ref)(x, w, bias, res, displace)


@functools.lru_cache(maxsize=None)
def exact_reference(name):
    """fp64 result of the exact family (integers).  Computed once per case; callers must not modify it."""
    return reference_of(CASES[name], *exact_inputs(name))


@functools.lru_cache(maxsize=None)
def randn_reference(name):
    return reference_of(CASES[name], *randn_inputs(name))


def exact_bound(name):
    """the largest value any partial sum of the case can reach in any order: sum |x| |w| + |bias| + |res|"""
    c = CASES[name]
    x, w, bias, res = exact_inputs(name)
    return reference_of(c, x.abs(), w.abs(), bias.abs(), None if res is None else res.abs()).max().item()


def output_tiles(c):
    """(row slice, column slice) of every 128 x 128 block of the [positions, Cout] output: the 128-row kernel's tiles, and every 256-row
    tile of the producer / consumer kernel is two of them"""
    M = positions(c)
    return [(slice(r, min(r + 128, M)), slice(n, min(n + 128, c.Cout))) for r in range(0, M, 128) for n in range(0, c.Cout, 128)]
