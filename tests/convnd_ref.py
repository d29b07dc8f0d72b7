"""fp64 references, an exact input family and the case list for the UNet's implicit-GEMM convolutions (csrc/convnd.hip: convnd_cl_kernel,
128 x 128 tiles; convnd320_kernel, 128 x 320 tiles, persistent, loader / multiplier waves; conv_dw_kernel, 128 x 128 weight-gradient
tiles with position splits over fp32 atomics; conv_dw320_kernel, 320-row weight-gradient tiles with the bias gradient folded in).

  * conv_ref / conv_dw_ref / conv_db_ref / conv_dx_ref / conv_dx_zero_insert_ref: the formula at the top of convnd.hip restated with explicit
    loops over the taps on zero-padded fp64 tensors.  No F.conv* here: tests/test_convnd_cpu.py pins these loops to F.conv3d and autograd,
    so the two stay independent.  conv_dx_ref is the adjoint (every tap scatters dy W into the padded input); conv_dx_zero_insert_ref is the
    stride-2 input gradient as the UNet computes it: row_map mode 2 (zero insertion) followed by the stride-1 convolution with the flipped,
    channel-swapped weight.  `displace` = (tap, offsets) makes ONE tap read at other offsets (a deliberately wrong convolution).
  * exact_inputs: x and dy integers in [-2, 2], weights in {-1, 0, 1}, bias multiples of 4 up to 128, residual multiples of 8 up to 512
    (all exact in bf16), sbias fp32 multiples of 0.25 up to 16, dW / dbias buffers pre-filled with integers in [-8, 8].  THE RULE: every
    term is a multiple of 0.25 and every partial sum, in any order and with every addend taken by magnitude, stays below 2^22 (forward:
    4 x bound < 2^24) resp. 2^24 (weight and bias gradient, integers, the second accumulating call included) -- so fp32 accumulation is
    exact whatever the order: MFMA K order, position splits, atomics.  Both forward epilogues (convnd_cl_kernel and convnd320_kernel) are
    fp32 `v + bias`, `+= sbias`, `+= res` and ONE pack2 (round-to-nearest-even): the stored bf16 must equal round_bf16(reference) bit
    for bit, the fp32 gradients the reference itself.  Residuals push results past 256, where bf16 holds even integers only, and sbias adds
    quarters, so the one rounding -- ties included -- is exercised, not just the sum.
  * CASES: the smallest shapes at which each thing can go wrong, each with the plans it must get under a forced kernel on a device with 256
    CUs (MI355X; also what the library assumes without a device), written down by hand from the tiling rules:
      forward, 128 x 128:  tiles = grid = ceil(M / 128) ceil(Cout / 128)                                   (M = output positions)
      forward, 128 x 320:  tiles = ceil(M / 128) Cout / 320, column tile inner (tile = nbn * row tile + column tile); grid = min(tiles,
                           slots or CUs); workgroup s walks tiles s, s + grid, ...
      dW, 128 x 128:       tiles = ceil(Cout / 128) ceil(taps Cin / 128); splits = min(ceil(512 / tiles), ceil(M / 512)), m_chunk =
                           ceil(M / splits) rounded up to 64, splits = ceil(M / m_chunk); dbias by the column-sum kernel
      dW, 320 rows:        tiles = Cout / 320 ceil(taps Cin / 128); the fewest s <= max(1, M // 256) with tiles s <= 1024 that fills >= 90 % of
                           whole passes of 256, else the best filled; m_chunk = ceil(M / s) rounded up to 32; dbias folded in
    tests/test_convnd_gpu.py imports them.
  * REAL_CONVS: every convolution of the VideoCrafter2 UNet at 320 x 512 x 16 (latent 16 x 40 x 64), one sample.
Pure torch, no GPU: the CPU and the GPU tests draw identical tensors from a seed."""
import functools
from collections import namedtuple

import torch

BF = torch.bfloat16
LIMIT = 1 << 24
K33, P33 = (1, 3, 3), (0, 1, 1)
K311, P311 = (3, 1, 1), (1, 0, 0)
K111, P111 = (1, 1, 1), (0, 0, 0)
MARGIN = 1          # spare zero lines around the padded input, so that a displaced tap may read one step outside every real tap


def round_bf16(t):
    """fp64 multiples of 0.25 below 2^22 -> bf16, one round-to-nearest-even (fp64 -> fp32 is exact for them; torch's fp32 -> bf16 is RNE)"""
    return t.float().to(BF)


def out_hw(H, W, k, pad, stride):
    return (H + 2 * pad[1] - k[1]) // stride + 1, (W + 2 * pad[2] - k[2]) // stride + 1


def taps_of(k):
    return [(dt, dh, dw) for dt in range(k[0]) for dh in range(k[1]) for dw in range(k[2])]


def _padded(x, pad):
    N, T, H, W, C = x.shape
    m = [p + MARGIN for p in pad]
    xp = torch.zeros(N, T + 2 * m[0], H + 2 * m[1], W + 2 * m[2], C, dtype=torch.float64)
    xp[:, m[0]:m[0] + T, m[1]:m[1] + H, m[2]:m[2] + W] = x
    return xp


def _tap_slices(off, T, Ho, Wo, stride):
    """index of the padded tensor that output position (t, ho, wo) reads through a tap at offsets off = (dt, dh, dw)"""
    et, eh, ew = (o + MARGIN for o in off)
    return (slice(None), slice(et, et + T), slice(eh, eh + stride * (Ho - 1) + 1, stride), slice(ew, ew + stride * (Wo - 1) + 1, stride))


def _tap_rows(xp, off, T, Ho, Wo, stride):
    return xp[_tap_slices(off, T, Ho, Wo, stride)].reshape(-1, xp.shape[-1])


def conv_ref(x, w, k, pad, stride=1, bias=None, sbias=None, res=None, displace=None):
    """x [N,T,H,W,Cin], w [Cout,Cin,KT,KH,KW] -> fp64 [N,T,Ho,Wo,Cout]:
    y[n,t,ho,wo,:] = bias + sbias[n] + res + sum_{dt,dh,dw} w[:,:,dt,dh,dw] x[n, t+dt-pt, ho s+dh-ph, wo s+dw-pw, :], zeros outside.
    displace = ((dt, dh, dw), (et, eh, ew)): that one tap reads at offsets (et, eh, ew), each in -1 .. K (a deliberately wrong convolution)"""
    x, w = x.double(), w.double()
    N, T, H, W, _ = x.shape
    Ho, Wo = out_hw(H, W, k, pad, stride)
    xp = _padded(x, pad)
    y = torch.zeros(N * T * Ho * Wo, w.shape[0], dtype=torch.float64)
    for tap in taps_of(k):
        off = displace[1] if displace is not None and displace[0] == tap else tap
        y += _tap_rows(xp, off, T, Ho, Wo, stride) @ w[:, :, tap[0], tap[1], tap[2]].t()
    y = y.view(N, T, Ho, Wo, -1)
    if bias is not None:
        y = y + bias.double()
    if sbias is not None:
        y = y + sbias.double()[:, None, None, None, :]
    if res is not None:
        y = y + res.double()
    return y


def conv_dw_ref(dy, x, k, pad, stride=1, rows=None):
    """weight gradient in the packed layout: fp64 [Cout, taps * Cin], dW[co, tap, ci] = sum_m dy[m, co] x[shift(m, tap), ci].
    rows: sum over the first `rows` output positions only (a sum that drops its last rows)"""
    dy, x = dy.double(), x.double()
    N, T, H, W, Cin = x.shape
    Ho, Wo = dy.shape[2], dy.shape[3]
    assert (Ho, Wo) == out_hw(H, W, k, pad, stride)
    xp = _padded(x, pad)
    d2 = dy.reshape(-1, dy.shape[-1])[:rows]
    return torch.cat([d2.t() @ _tap_rows(xp, tap, T, Ho, Wo, stride)[:rows] for tap in taps_of(k)], dim=1)


def conv_db_ref(dy):
    return dy.double().reshape(-1, dy.shape[-1]).sum(0)


def conv_dx_ref(dy, w, k, pad, stride, H, W):
    """input gradient, the adjoint of conv_ref: every tap adds dy W[:, :, tap] to the input positions it read.  fp64 [N,T,H,W,Cin]"""
    dy, w = dy.double(), w.double()
    N, T, Ho, Wo, Cout = dy.shape
    dxp = _padded(torch.zeros(N, T, H, W, w.shape[1], dtype=torch.float64), pad)
    d2 = dy.reshape(-1, Cout)
    for tap in taps_of(k):
        dxp[_tap_slices(tap, T, Ho, Wo, stride)] += (d2 @ w[:, :, tap[0], tap[1], tap[2]]).view(N, T, Ho, Wo, -1)
    m = [p + MARGIN for p in pad]
    return dxp[:, m[0]:m[0] + T, m[1]:m[1] + H, m[2]:m[2] + W].clone()


def zero_insert(dy):
    """row_map mode 2: [N,T,Ho,Wo,C] -> [N,T,2 Ho,2 Wo,C], dy at the even lines / columns, zeros elsewhere"""
    N, T, Ho, Wo, C = dy.shape
    z = torch.zeros(N, T, 2 * Ho, 2 * Wo, C, dtype=dy.dtype)
    z[:, :, ::2, ::2] = dy
    return z


def dx_weight(w):
    """[Cout,Cin,KT,KH,KW] -> the weight of the input-gradient convolution [Cin,Cout,KT,KH,KW]: taps flipped, channels swapped"""
    return w.flip((2, 3, 4)).transpose(0, 1).contiguous()


def conv_dx_zero_insert_ref(dy, w, k, pad):
    """the stride-2 input gradient as the UNet computes it (H = 2 Ho, W = 2 Wo): zero insertion, then the stride-1 convolution with the
    flipped, channel-swapped weight"""
    return conv_ref(zero_insert(dy.double()), dx_weight(w), k, pad, 1)


# ------------------------------------------------------------------------------------------------ cases
# k / pad / stride: the convolution; res / sb: the forward adds a residual / a per-sample bias; slots: the persistent-grid cap given to
# conv_set_tile for the 128 x 320 forward run (0 = the device's own).  pads = (x, y, residual, dy) extra elements per position: the inputs'
# hold NaN, the outputs' are poisoned and checked bit for bit.  Plans (module docstring): f128 = tiles of the 128 x 128 forward launch,
# f320 = (grid, tiles, most tiles per workgroup) of the 128 x 320 one or None where Cout % 320; d128 / d320 = (tiles, splits, m_chunk) of the
# weight-gradient launches.  run: f forward, x input gradient, w weight gradient.  randn: the case also runs randn inputs on every kernel.
Case = namedtuple("Case", "N T H W Cin Cout k pad stride res sb slots pads f128 f320 d128 d320 run randn")


def _c(N, T, H, W, Cin, Cout, k=K33, pad=P33, stride=1, res=False, sb=False, slots=0, pads=(0, 0, 0, 0), f128=None, f320=None, d128=None,
       d320=None, run="fxw", randn=False):
    return Case(N, T, H, W, Cin, Cout, k, pad, stride, res, sb, slots, pads, f128, f320, d128, d320, run, randn)


CASES = {
    # ---- samples inside one 128-row tile: sbias row, n and t change mid-tile.  126 positions = 3 samples of 42, T = 1, Wo = 7
    "straddle3": _c(3, 1, 6, 7, 64, 64, res=True, sb=True, f128=1, d128=(5, 1, 128), randn=True),
    # Wo = 1, Ho = 11: 66 positions, two samples of three frames
    "wo_1": _c(2, 3, 11, 1, 64, 64, sb=True, f128=1, d128=(5, 1, 128)),
    # H = W = 1, T = 13: Ho Wo = 1, a sample is 13 rows; temporal taps cross no sample boundary
    "hw_1": _c(2, 13, 1, 1, 64, 64, K311, P311, res=True, sb=True, f128=1, d128=(2, 1, 64)),
    # primes: T = 3, Ho = 7, Wo = 11 (Ho Wo = 77), 462 positions = 3.6 tiles
    "primes": _c(2, 3, 7, 11, 64, 64, K311, P311, sb=True, f128=4, d128=(2, 1, 512)),
    # ---- rows at exactly 128, 129 (three samples of 43, H = 1) and 255 (T = 5)
    "rows_128": _c(1, 2, 8, 8, 64, 64, f128=1, d128=(5, 1, 128)),
    "rows_129": _c(3, 1, 1, 43, 64, 64, res=True, sb=True, f128=2, d128=(5, 1, 192)),
    "rows_255": _c(1, 5, 3, 17, 64, 64, K311, P311, res=True, f128=2, d128=(2, 1, 256)),
    # ---- column tiles: 4 (the out convolution; dy rows are 8 wide), 132 (ragged second tile), 320 (third tile 5/8 empty), 640 (nbn = 2)
    "cout_4": _c(1, 2, 6, 6, 64, 4, res=True, pads=(0, 4, 4, 4), f128=1, d128=(5, 1, 128), run="fw"),
    "cout_132": _c(2, 3, 5, 7, 64, 132, res=True, sb=True, pads=(8, 4, 8, 4), f128=4, d128=(10, 1, 256), run="fw"),
    # 210 positions: the 320-row dW kernel forced below 256 rows -- one split, the last 32-row K-tile holds 18
    "cout_320": _c(2, 3, 5, 7, 64, 320, res=True, sb=True, f128=6, f320=(2, 2, 1), d128=(15, 1, 256), d320=(5, 1, 224), randn=True),
    "cout_640": _c(2, 3, 5, 7, 64, 640, res=True, f128=10, f320=(4, 4, 1), d128=(25, 1, 256), d320=(10, 1, 224)),
    # ---- K axis: two K-tiles per tap on the 128 kernel; (tap, ci) axis 1728 = 13.5 tiles, tile 1 straddles taps 0 and 1 (Cin = 192)
    "cin_128": _c(2, 3, 5, 7, 128, 64, sb=True, f128=2, d128=(9, 1, 256)),
    "cin_192": _c(2, 1, 5, 5, 192, 64, res=True, f128=1, d128=(14, 1, 64)),
    # ten 32-channel K-tiles per tap on the 320 kernel; (tap, ci) axis 2880 = 22.5 tiles; the input gradient runs on the 320 kernel too
    "cin_320": _c(1, 2, 9, 8, 320, 320, res=True, sb=True, f128=6, f320=(2, 2, 1), d128=(69, 1, 192), d320=(23, 1, 160), randn=True),
    # temporal taps, Cin = 64: the (tap, ci) axis is 192 wide, its second 128-column tile half empty and inside tap 1 .. 2
    "k311_320": _c(2, 4, 6, 5, 64, 320, K311, P311, res=True, f128=6, f320=(2, 2, 1), d128=(6, 1, 256), d320=(2, 1, 256)),
    # ---- the three tap shapes at stride 2, odd and even H / W (the input gradient by zero insertion needs even ones)
    "s2_k33_odd": _c(2, 2, 9, 7, 64, 64, stride=2, res=True, sb=True, f128=1, d128=(5, 1, 128), run="fw", randn=True),
    "s2_k33_even": _c(2, 2, 8, 12, 64, 64, stride=2, sb=True, f128=1, d128=(5, 1, 128)),
    "s2_k311_odd": _c(2, 3, 7, 5, 64, 64, K311, P311, 2, res=True, f128=1, d128=(2, 1, 128), run="fw"),
    "s2_k311_even": _c(2, 3, 6, 8, 64, 64, K311, P311, 2, sb=True, f128=1, d128=(2, 1, 128)),
    "s2_k111_odd": _c(3, 2, 5, 9, 64, 64, K111, P111, 2, res=True, sb=True, f128=1, d128=(1, 1, 128), run="fw"),
    "s2_k111_even": _c(3, 2, 4, 10, 64, 64, K111, P111, 2, f128=1, d128=(1, 1, 64)),
    "k111": _c(1, 1, 4, 4, 192, 320, K111, P111, res=True, f128=3, f320=(1, 1, 1), d128=(6, 1, 64), d320=(2, 1, 32)),
    # stride 2 on the 320 kernels, forward, zero-insertion input gradient and dW: 96 output positions, 384 input positions
    "s2_320": _c(2, 2, 8, 12, 320, 320, stride=2, res=True, sb=True, f128=3, f320=(1, 1, 1), d128=(69, 1, 128), d320=(23, 1, 96)),
    # ---- convnd320_kernel hand-over, slots = 8.  2500 positions x 320 columns = 20 tiles: workgroups walk 3,3,3,3,2,2,2,2
    "handover_320": _c(2, 5, 10, 25, 64, 320, slots=8, f128=60, f320=(8, 20, 3), d128=(15, 5, 512), d320=(5, 9, 288), randn=True),
    "handover_320_res": _c(2, 5, 10, 25, 64, 320, res=True, sb=True, slots=8, pads=(8, 4, 12, 8), f128=60, f320=(8, 20, 3), d128=(15, 5, 512),
                           d320=(5, 9, 288), randn=True),
    # 1250 positions x 640 columns = 10 x 2 = 20 tiles: tile % 2 alternates inside a row tile, tile + 8 keeps its column tile
    "handover_640": _c(2, 5, 5, 25, 64, 640, slots=8, f128=50, f320=(8, 20, 3), d128=(25, 3, 448), d320=(10, 4, 320)),
    "handover_640_res": _c(2, 5, 5, 25, 64, 640, res=True, sb=True, slots=8, f128=50, f320=(8, 20, 3), d128=(25, 3, 448), d320=(10, 4, 320)),
    # slots = 7: tile + 7 lands on the OTHER column tile; workgroups walk 3,3,3,3,3,3,2
    "handover_640_odd": _c(2, 5, 5, 25, 64, 640, res=True, sb=True, slots=7, pads=(8, 8, 4, 0), f128=50, f320=(7, 20, 3), d128=(25, 3, 448),
                           d320=(10, 4, 320), run="f"),
    # the device's own grid: 33 000 positions x 320 columns = 258 tiles on 256 workgroups, two of which walk two tiles.  dW by the rule
    # (>= 2048 rows): 2 tiles x 116 splits fill 232 of 256; 288-row chunks make 115 splits, the last of 168 rows
    "device_grid": _c(1, 8, 55, 75, 64, 320, K311, P311, res=True, sb=True, f128=774, f320=(256, 258, 2), d128=(6, 65, 512), d320=(2, 115, 288),
                      run="fw"),
    # ---- conv_dw_kernel: 1100 positions = 3 splits of 384, the last 332 rows = 5 K-tiles and 12 rows
    "dw_splits": _c(2, 2, 11, 25, 64, 64, sb=True, f128=9, d128=(5, 3, 384)),
    # ---- conv_dw320_kernel by the rule: 2250 positions, 8 splits of 288, the last 234 rows = 7 K-tiles and 10 rows
    "dw320_rule": _c(1, 3, 30, 25, 64, 320, res=True, f128=54, f320=(18, 18, 1), d128=(15, 5, 512), d320=(5, 8, 288), run="fw"),
    # ---- the Linear weight gradient (one tap, rows = W): test_linear_dw_any_size's small sizes, P = 8 among them
    "lin_1000_320_320": _c(1, 1, 1, 1000, 320, 320, K111, P111, pads=(8, 0, 0, 8), d128=(9, 2, 512), d320=(3, 3, 352), run="w"),
    "lin_77_64_1024": _c(1, 1, 1, 77, 1024, 64, K111, P111, d128=(8, 1, 128), run="w"),
    "lin_300_8_72": _c(1, 1, 1, 300, 72, 8, K111, P111, pads=(0, 0, 0, 8), d128=(1, 1, 320), run="w"),
    "lin_200_8_320": _c(1, 1, 1, 200, 320, 8, K111, P111, d128=(3, 1, 256), run="w"),
}
FWD_CASES = tuple(n for n, c in CASES.items() if "f" in c.run)
DX_CASES = tuple(n for n, c in CASES.items() if "x" in c.run)
DW_CASES = tuple(n for n, c in CASES.items() if "w" in c.run)
RANDN_CASES = tuple(n for n, c in CASES.items() if c.randn)
KERNELS = {"k128": 1, "k320": 2}


def case_hw(c):
    return out_hw(c.H, c.W, c.k, c.pad, c.stride)


def positions(c):
    Ho, Wo = case_hw(c)
    return c.N * c.T * Ho * Wo


def dx_plan(c, kernel):
    """plan of the input-gradient launch: the stride-1 forward kernel over the N T H W INPUT positions with Cout and Cin swapped, on the
    device's own grid.  (kernel, grid, tiles, tiles per workgroup), or None where the 128 x 320 kernel cannot run (Cin % 320)"""
    nbm = -(-(c.N * c.T * c.H * c.W) // 128)
    if kernel == 1:
        t = nbm * -(-c.Cin // 128)
        return (1, t, t, 1)
    if c.Cin % 320:
        return None
    t = nbm * (c.Cin // 320)
    return (2, min(t, 256), t, -(-t // min(t, 256)))


def fwd_pairs():
    """(case, kernel name) of every forward run: the 128 x 320 kernel only where Cout % 320 == 0"""
    return [(n, kn) for n in FWD_CASES for kn in KERNELS if kn == "k128" or CASES[n].f320 is not None]


def dx_pairs():
    return [(n, kn) for n in DX_CASES for kn, km in KERNELS.items() if dx_plan(CASES[n], km) is not None]


def dw_pairs():
    return [(n, kn) for n in DW_CASES for kn in KERNELS if kn == "k128" or CASES[n].d320 is not None]


def _seed(name):
    return 2000 + list(CASES).index(name)


@functools.lru_cache(maxsize=None)
def exact_inputs(name):
    """-> dict of fp32 tensors holding values exact in bf16 (sbias: in fp32): x [N,T,H,W,Cin], w [Cout,Cin,KT,KH,KW], bias [Cout], sbias
    [N,Cout] | None, res like y | None, dy like y, dw_fill [Cout, taps Cin], db_fill [Cout]"""
    c = CASES[name]
    g = torch.Generator().manual_seed(_seed(name))
    Ho, Wo = case_hw(c)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    d = {"x": ri(-2, 2, (c.N, c.T, c.H, c.W, c.Cin)), "w": ri(-1, 1, (c.Cout, c.Cin) + c.k), "bias": 4.0 * ri(-32, 32, (c.Cout,))}
    d["sbias"] = 0.25 * ri(-64, 64, (c.N, c.Cout)) if c.sb else None
    d["res"] = 8.0 * ri(-64, 64, (c.N, c.T, Ho, Wo, c.Cout)) if c.res else None
    d["dy"] = ri(-2, 2, (c.N, c.T, Ho, Wo, c.Cout))
    d["dw_fill"] = ri(-8, 8, (c.Cout, c.k[0] * c.k[1] * c.k[2] * c.Cin))
    d["db_fill"] = ri(-8, 8, (c.Cout,))
    return d


@functools.lru_cache(maxsize=None)
def randn_inputs(name):
    """the same tensors with randn values rounded to bf16, scaled as test_conv_cl_forward_input_grad_weight_grad scales them"""
    c = CASES[name]
    g = torch.Generator().manual_seed(7 * _seed(name))
    Ho, Wo = case_hw(c)
    rb = lambda t: t.to(BF).float()
    taps = c.k[0] * c.k[1] * c.k[2]
    d = {"x": rb(torch.randn(c.N, c.T, c.H, c.W, c.Cin, generator=g)),
         "w": rb(torch.randn((c.Cout, c.Cin) + c.k, generator=g) / (taps * c.Cin) ** 0.5),
         "bias": rb(torch.randn(c.Cout, generator=g) * 0.1)}
    d["sbias"] = torch.randn(c.N, c.Cout, generator=g) * 0.1 if c.sb else None
    d["res"] = rb(torch.randn(c.N, c.T, Ho, Wo, c.Cout, generator=g)) if c.res else None
    d["dy"] = rb(torch.randn(c.N, c.T, Ho, Wo, c.Cout, generator=g))
    return d


def forward_of(c, d, displace=None):
    return conv_ref(d["x"], d["w"], c.k, c.pad, c.stride, d["bias"], d["sbias"], d["res"], displace)


def input_grad_of(c, d):
    """the input gradient the way the UNet computes it: the stride-1 kernel on dy, or on the zero-inserted dy, with the flipped weight"""
    if c.stride == 1:
        return conv_ref(d["dy"], dx_weight(d["w"]), c.k, c.pad, 1)
    return conv_dx_zero_insert_ref(d["dy"], d["w"], c.k, c.pad)


# Computed once per case; callers must not modify the results.
@functools.lru_cache(maxsize=None)
def exact_forward(name):
    return forward_of(CASES[name], exact_inputs(name))


@functools.lru_cache(maxsize=None)
def exact_input_grad(name):
    return input_grad_of(CASES[name], exact_inputs(name))


@functools.lru_cache(maxsize=None)
def exact_weight_grad(name):
    """(dW [Cout, taps Cin], dbias [Cout]) fp64"""
    c, d = CASES[name], exact_inputs(name)
    return conv_dw_ref(d["dy"], d["x"], c.k, c.pad, c.stride), conv_db_ref(d["dy"])


@functools.lru_cache(maxsize=None)
def randn_refs(name):
    """(forward, input gradient | None, dW, dbias) fp64 of the randn inputs"""
    c, d = CASES[name], randn_inputs(name)
    dx = input_grad_of(c, d) if "x" in c.run else None
    return forward_of(c, d), dx, conv_dw_ref(d["dy"], d["x"], c.k, c.pad, c.stride), conv_db_ref(d["dy"])


def exact_bounds(name):
    """the largest value any partial sum can reach in any order, every addend by magnitude: (forward, input gradient, weight gradient with
    the fill and a second accumulating call, bias gradient likewise)"""
    c = CASES[name]
    a = {k: (None if v is None else v.abs()) for k, v in exact_inputs(name).items()}
    fwd = forward_of(c, a).max().item() if "f" in c.run else 0.0
    dx = input_grad_of(c, a).max().item() if "x" in c.run else 0.0
    dw = (a["dw_fill"].double() + 2 * conv_dw_ref(a["dy"], a["x"], c.k, c.pad, c.stride)).max().item()
    db = (a["db_fill"].double() + 2 * conv_db_ref(a["dy"])).max().item()
    return fwd, dx, dw, db


def _reads_input(c, off):
    """does a tap at offsets off read any real input position (not only zero padding) from some output position"""
    Ho, Wo = case_hw(c)
    for o, p, ext, n, s in zip(off, c.pad, (c.T, c.H, c.W), (c.T, Ho, Wo), (1, c.stride, c.stride)):
        if not any(0 <= i * s + o - p < ext for i in range(n)):
            return False
    return True


def displaced(c):
    """for every tap one wrong read position: ((dt, dh, dw), (et, eh, ew)) pairs.  The tap is moved by one step, the first of w + 1, w - 1,
    h + 1, h - 1, t + 1, t - 1 after which it or the true tap reads real input (at W = 1 or H = 1 a tap of the 3 x 3 kernel may read nothing
    but padding, and so may its neighbour)"""
    out = []
    for tap in taps_of(c.k):
        for axis, step in ((2, 1), (2, -1), (1, 1), (1, -1), (0, 1), (0, -1)):
            off = tuple(o + (step if i == axis else 0) for i, o in enumerate(tap))
            if (c.T, c.H, c.W)[axis] + c.k[axis] > 2 and (_reads_input(c, tap) or _reads_input(c, off)):
                out.append((tap, off))
                break
        else:
            raise AssertionError(f"tap {tap} cannot be displaced")
    return out


# ------------------------------------------------------------------------------------------------ the real UNet
def unet_convs(structure, H, W):
    """every convolution a forward of the UNet launches through conv_cl, from vt355.unet.build_structure's layer list, on an H x W latent:
    (H, W of the convolution's INPUT, Cin, Cout, kernel, stride) in launch order.  conv_in sees its 4 channels padded to 64; a ResBlock is
    two 3x3 convolutions and, with tconv, the four (3,1,1) ones of its TemporalConvBlock (its 1x1 skip connection is a Linear)"""
    out = []
    for block in structure.input + [structure.middle] + structure.output:
        for l in block:
            if l.kind == "conv_in":
                out.append((H, W, 64, l.cout, K33, 1))
            elif l.kind == "res":
                out += [(H, W, l.cin, l.cout, K33, 1), (H, W, l.cout, l.cout, K33, 1)] + ([(H, W, l.cout, l.cout, K311, 1)] * 4 if l.tconv else [])
            elif l.kind == "down":
                out.append((H, W, l.c, l.c, K33, 2))
                H, W = H // 2, W // 2
            elif l.kind == "up":
                H, W = 2 * H, 2 * W
                out.append((H, W, l.c, l.c, K33, 1))
    return out + [(H, W, structure.out_ch, 4, K33, 1)]


# Every distinct convolution of the VideoCrafter2 UNet (model_channels 320, channel_mult (1, 2, 4, 4), two ResBlocks per level, a
# TemporalConvBlock behind every ResBlock) at 320 x 512 x 16 = a 16 x 40 x 64 latent, ONE sample, with what conv_set_tile(0) gives it on 256
# CUs: (H, W of the input, Cin, Cout, kernel, stride, how many layers) -> (forward kernel, input-gradient kernel, dW kernel, dW splits);
# 1 = the 128 x 128 kernels, 2 = the 320-wide ones.  One sample fills the 128 x 320 forward kernel's passes (>= 80 % of a multiple of 256
# tiles) only for the input gradient of 960 -> 320 at 40 x 64 (960 tiles of 1024); dW takes the 320-row kernel from 2048 positions on.
REAL_CONVS = {
    (40, 64, 64, 320, K33, 1, 1): (1, 1, 2, 46),          # conv_in
    (40, 64, 320, 320, K33, 1, 7): (1, 1, 2, 11),
    (40, 64, 320, 320, K311, 1, 20): (1, 1, 2, 29),
    (40, 64, 320, 320, K33, 2, 1): (1, 1, 2, 11),         # Downsample
    (20, 32, 320, 640, K33, 1, 1): (1, 1, 2, 11),
    (20, 32, 640, 640, K33, 1, 6): (1, 1, 2, 8),
    (20, 32, 640, 640, K311, 1, 20): (1, 1, 2, 8),
    (20, 32, 640, 640, K33, 2, 1): (1, 1, 2, 8),
    (10, 16, 640, 1280, K33, 1, 1): (1, 1, 2, 4),
    (10, 16, 1280, 1280, K33, 1, 7): (1, 1, 2, 2),        # five ResBlock convolutions and two Upsample ones
    (10, 16, 1280, 1280, K311, 1, 20): (1, 1, 2, 2),
    (10, 16, 1280, 1280, K33, 2, 1): (1, 1, 1, 1),        # 1280 output positions: below 2048
    (5, 8, 1280, 1280, K33, 1, 11): (1, 1, 1, 1),
    (5, 8, 1280, 1280, K311, 1, 28): (1, 1, 1, 2),
    (5, 8, 2560, 1280, K33, 1, 3): (1, 1, 1, 1),
    (10, 16, 2560, 1280, K33, 1, 2): (1, 1, 2, 1),
    (10, 16, 1920, 1280, K33, 1, 1): (1, 1, 2, 1),
    (20, 32, 1280, 1280, K33, 1, 1): (1, 1, 2, 2),        # Upsample
    (20, 32, 1920, 640, K33, 1, 1): (1, 1, 2, 3),
    (20, 32, 1280, 640, K33, 1, 1): (1, 1, 2, 4),
    (20, 32, 960, 640, K33, 1, 1): (1, 1, 2, 7),
    (40, 64, 640, 640, K33, 1, 1): (1, 1, 2, 8),          # Upsample
    (40, 64, 960, 320, K33, 1, 1): (1, 2, 2, 7),
    (40, 64, 640, 320, K33, 1, 2): (1, 1, 2, 11),
    (40, 64, 320, 4, K33, 1, 1): (1, 1, 1, 23),           # out: 4 channels in 8-wide dy rows; its input gradient pads them to 64
}


def real_unet_structure():
    """vt355.unet.build_structure of the real configuration (oracle/unet_oracle.py's UNetConfig defaults are VideoCrafter2's)"""
    from unet_oracle import UNetConfig
    from vt355.unet import build_structure
    cfg = UNetConfig()
    assert (cfg.model_channels, tuple(cfg.channel_mult), cfg.num_res_blocks, cfg.temporal_conv) == (320, (1, 2, 4, 4), 2, True)
    return build_structure(cfg)


def real_unet_choices(ops, T=16):
    """REAL_CONVS as the library's plan queries see it under the current conv_set_tile setting (ops = vt355.ops); the input gradient is the
    stride-1 convolution over the input positions with dy's channels padded to a whole K-tile of 64, as UNet.conv_bwd runs it"""
    got = {}
    for (H, W, Cin, Cout, k, stride, n) in REAL_CONVS:
        pad = P33 if k == K33 else P311
        fwd = ops.conv_plan(1, T, H, W, Cin, Cout, k, pad, stride)[0]
        dxk = ops.conv_plan(1, T, H, W, -(-Cout // 64) * 64, Cin, k, pad, 1)[0]
        dw = ops.conv_dw_plan(1, T, H, W, Cin, Cout, k, pad, stride, lddy=-(-Cout // 8) * 8)
        got[(H, W, Cin, Cout, k, stride, n)] = (fwd, dxk, dw[0], dw[2])
    return got
