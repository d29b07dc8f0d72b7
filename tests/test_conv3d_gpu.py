"""vt_causal_conv3d_cl, vt_downsample_conv2d_cl and vt_causal_conv3d_in8_cl against the fp64 tap loops of tests/conv3d_ref.py, on BOTH kernels
of csrc/conv3d.hip: conv3d_cl_kernel (128-row tiles) and conv3d_pc_kernel (256-row tiles, persistent, loader / multiplier waves, a three
stage LDS ring that runs across output tiles), which the shape rule takes only from 4096 tiles on and which tests/test_kernels_gpu.py
therefore never reaches.  conv3d_set_kernel forces the kernel and, with slots = 8, a grid small enough that workgroups walk several tiles
at a few thousand positions; every case first asserts through conv3d_plan that the launch is the kernel, grid and tiles per workgroup it is
named after -- a case that silently ran the other kernel fails.

Every case runs the exact family (integers: the fp32 sums are exact in any order, one round-to-nearest-even in pack2) and is compared BIT
FOR BIT with the once-rounded fp64 reference.  Outputs are poisoned buffers, pad columns must still hold the poison, input pads hold NaN.
A subset also runs randn inputs on both kernels at the bars of test_causal_conv3d_channels_last (rtol 1e-2, atol 1e-2 max|ref|), and the two
kernels' randn outputs are compared with each other: same MFMA shape, same K order -- they are bit-equal, and that is asserted.

The shape rule's own choices (conv3d_set_kernel(0), MI355X, 256 CUs) for every convolution of the real models, one sample
(conv3d_ref.REAL_CONVS; T x H x W is the convolution's input):
  encoder, 49 x 480 x 720                                                   decoder, latent 13 x 60 x 90
  down.0  128 -> 128   49 x 480 x 720   128-row (one column tile)           conv_in 64 -> 512   13 x 60 x 90     128-row (1100 tiles)
  down.0  downsample   25 x 480 x 720   128-row (one column tile)           mid, up.3 512 -> 512  13 x 60 x 90   128-row (1100 tiles)
  down.1  128 -> 256   25 x 240 x 360   PRODUCER / CONSUMER (16 876 tiles)  up.2  512 -> 256   25 x 120 x 180    PRODUCER / CONSUMER (4220)
  down.1  256 -> 256   25 x 240 x 360   PRODUCER / CONSUMER (16 876 tiles)  up.2  256 -> 256   25 x 120 x 180    PRODUCER / CONSUMER (4220)
  down.1  downsample   13 x 240 x 360   128-row (2194 tiles)                up.1  256 -> 256   49 x 240 x 360    PRODUCER / CONSUMER (33 076)
  down.2  256 -> 256   13 x 120 x 180   128-row (2194 tiles)                up.0  256 -> 128   49 x 480 x 720    128-row (one column tile)
  down.2  downsample   13 x 120 x 180   128-row (550 tiles)                 up.0  128 -> 128   49 x 480 x 720    128-row (one column tile)
  down.3  256 -> 512, 512 -> 512, mid  13 x 60 x 90  128-row (1100 tiles)   conv_out 128 -> 4  49 x 480 x 720    128-row (one column tile)
  conv_out 512 -> 32   13 x 60 x 90     128-row (one column tile)
The three channel pairs that take the producer / consumer kernel (128 -> 256, 256 -> 256, 512 -> 256) have a forced small case each
(pair_*).  The downsample never takes it in the real models; it is instantiated, reachable through the rule at other sizes, and tested."""
import pytest
import torch

import conv3d_ref as R
from parity import close, poisoned, untouched

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
KERNELS = {"rows128": 1, "pc": 2}


def _padded(t, pad, dev):
    """t [..., C] as a view into a poisoned buffer of [..., C + pad]: the pad holds NaN, which must reach no result"""
    buf = poisoned(tuple(t.shape[:-1]) + (t.shape[-1] + pad,), BF, dev)
    buf[..., :t.shape[-1]] = t.to(dev, BF)
    return buf[..., :t.shape[-1]]


def _forced(c, kernel):
    """force `kernel` for case c and assert the plan the case is named after; the caller restores the setting"""
    from vt355 import ops
    ops.conv3d_set_kernel(kernel, c.slots if kernel == 2 else 0)
    kt, stride = (1, 2) if c.op == "ds" else (3, 1)
    plan = ops.conv3d_plan(c.N, c.T, c.H, c.W, c.Cin, c.Cout, kt, stride, c.Cin + c.pads[0])
    want = (2,) + c.pc if kernel == 2 else (1, c.cl, c.cl, 1)
    assert plan == want, f"plan (kernel, grid, tiles, tiles per workgroup) {plan}, the case is written for {want}"


def _run(dev, c, inputs):
    """one launch of case c under the current kernel setting -> (y view [N,T,Ho,Wo,Cout], its whole buffer)"""
    from vt355 import ops
    x, w, bias, res = inputs
    Ho, Wo = R.out_hw(c)
    X = _padded(x, c.pads[0], dev)
    rd = None if res is None else _padded(res, c.pads[2], dev)
    ybuf = poisoned((c.N, c.T, Ho, Wo, c.Cout + c.pads[1]), BF, dev)
    y = ybuf[..., :c.Cout]
    wk = ops.pack_conv_weight(w).to(dev, BF)
    if c.op == "ds":
        ops.downsample_conv2d(X, wk, bias.to(dev, BF), y, residual=rd)
    else:
        ops.causal_conv3d(X, wk, bias.to(dev, BF), y, residual=rd)
    return y, ybuf


def _bits(t):
    return t.contiguous().view(torch.int16)


def _assert_bit_equal(y, want, what):
    got = y.cpu()
    if torch.equal(_bits(got), _bits(want)):
        return
    bad = _bits(got) != _bits(want)
    at = int(bad.flatten().int().argmax())
    rows = bad.view(-1, bad.shape[-1]).any(1).nonzero().flatten()
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the once-rounded fp64 reference, first at flat index "
                         f"{at} (got {got.flatten()[at].item()}, want {want.flatten()[at].item()}), in {rows.numel()} positions "
                         f"{rows[0].item()}..{rows[-1].item()}")


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", R.PC_CASES)
def test_exact(dev, name, kernel):
    """integer inputs: the stored bf16 must equal the fp64 reference rounded once to nearest-even, bit for bit, on either kernel"""
    from vt355 import ops
    c = R.CASES[name]
    want = R.round_bf16(R.exact_reference(name))
    try:
        _forced(c, KERNELS[kernel])
        y, ybuf = _run(dev, c, R.exact_inputs(name))
        torch.cuda.synchronize()
    finally:
        ops.conv3d_set_kernel(0, 0)
    _assert_bit_equal(y, want, f"{name} {kernel}")
    untouched(ybuf, (Ellipsis, slice(0, c.Cout)), f"{name} {kernel}: pad columns of y")


@pytest.mark.parametrize("name", R.IN8_CASES)
def test_exact_in8(dev, name):
    """the 8-channel first convolution (8 taps per K-tile, taps 27..31 and channels >= Cin zero) at the same edges, bit for bit"""
    from vt355 import ops
    c = R.CASES[name]
    x, w, bias, _ = R.exact_inputs(name)
    want = R.round_bf16(R.exact_reference(name))
    x8 = torch.zeros(c.N, c.T, c.H, c.W, 8, dtype=BF, device=dev)
    x8[..., :c.Cin] = x.to(dev, BF)
    ybuf = poisoned((c.N, c.T, c.H, c.W, c.Cout + 4), BF, dev)
    ops.causal_conv3d_in8(x8, ops.pack_conv_in8_weight(w).to(dev, BF), bias.to(dev, BF), ybuf[..., :c.Cout])
    torch.cuda.synchronize()
    _assert_bit_equal(ybuf[..., :c.Cout], want, name)
    untouched(ybuf, (Ellipsis, slice(0, c.Cout)), f"{name}: pad columns of y")


@pytest.mark.parametrize("name", R.RANDN_CASES)
def test_randn_on_both_kernels(dev, name):
    """randn inputs against the fp64 reference at the bars of test_causal_conv3d_channels_last on each kernel, and the two kernels against
    each other: 16x16x32 MFMA over the same K-tiles in the same order, fp32 epilogue, one rounding -- bit-equal"""
    from vt355 import ops
    c = R.CASES[name]
    ref = R.randn_reference(name)
    atol = 1e-2 * ref.abs().max().item()
    out = {}
    for kernel, mode in KERNELS.items():
        try:
            _forced(c, mode)
            y, ybuf = _run(dev, c, R.randn_inputs(name))
            torch.cuda.synchronize()
        finally:
            ops.conv3d_set_kernel(0, 0)
        close(y, ref, 1e-2, atol, f"{name} {kernel}")
        untouched(ybuf, (Ellipsis, slice(0, c.Cout)), f"{name} {kernel}: pad columns of y")
        out[kernel] = y.cpu()
    a, b = out["rows128"], out["pc"]
    ndiff = int((_bits(a) != _bits(b)).sum())
    print(f"{name}: {ndiff} of {a.numel()} elements differ between the kernels, max |diff| {(a.float() - b.float()).abs().max().item():.3g}")
    assert ndiff == 0


def test_shape_rule_choices_for_the_real_vae(dev):
    """conv3d_set_kernel(0): the kernel each convolution of the real encoder / decoder gets (the table in this file's docstring), and the
    small cases all stay on the 128-row kernel -- the producer / consumer kernel is the default nowhere it was not"""
    from vt355 import ops
    ops.conv3d_set_kernel(0, 0)
    got = [(what, ops.conv3d_plan(1, T, H, W, Cin, Cout, kt, stride)[0]) for what, T, H, W, Cin, Cout, kt, stride, _ in R.REAL_CONVS]
    assert got == [(r[0], r[8]) for r in R.REAL_CONVS]
    # the threshold itself, 256 -> 256 at 240 x 360: 4096 tiles = 2048 row tiles of 256 = 524 288 positions, between 6 and 7 frames
    assert ops.conv3d_plan(1, 7, 240, 360, 256, 256)[:3] == (2, 256, 4726)
    assert ops.conv3d_plan(1, 6, 240, 360, 256, 256)[0] == 1 and ops.conv3d_plan(1, 49, 240, 360, 256, 128)[0] == 1
    for c in (R.CASES[n] for n in R.PC_CASES):
        kt, stride = (1, 2) if c.op == "ds" else (3, 1)
        assert ops.conv3d_plan(c.N, c.T, c.H, c.W, c.Cin, c.Cout, kt, stride, c.Cin + c.pads[0]) == (1, c.cl, c.cl, 1)
