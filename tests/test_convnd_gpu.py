"""conv_cl (forward and input gradient), conv_dw_cl and linear_dw against the fp64 tap loops of tests/convnd_ref.py on ALL FOUR kernels of
csrc/convnd.hip: convnd_cl_kernel (128 x 128 tiles), convnd320_kernel (128 x 320 tiles, persistent: four loader waves run ahead across
output tiles through a five-stage LDS ring), conv_dw_kernel (128 x 128 weight-gradient tiles, position splits over fp32 atomics) and
conv_dw320_kernel (320-row tiles, the bias gradient folded in).  conv_set_tile forces the kernel and, with slots = 8 or 7, a grid small
enough that workgroups of convnd320_kernel walk three tiles at a few thousand positions; every case first asserts through conv_plan /
conv_dw_plan that the launch is the kernel, grid, tiles, splits and rows per split it is named after -- a case that silently ran the other
kernel fails.

Every case runs the exact family (convnd_ref: integers and quarters whose fp32 sums are exact in any order, atomics included; one
round-to-nearest-even in pack2) and is compared BIT FOR BIT with the once-rounded fp64 reference (bf16 outputs) or the reference itself
(fp32 dW / dbias, after a plain call into a poisoned buffer, after an accumulating call onto an integer pattern, and the bias gradient
after both).  Outputs are poisoned buffers, their pad columns must still hold the poison, input pads hold NaN.  A subset also runs randn
inputs on every kernel at the bars of test_conv_cl_forward_input_grad_weight_grad, and the kernels' randn outputs are compared with
each other: the two forward kernels issue the same 16 x 16 x 32 MFMAs over the same 32-channel steps in the same order (taps outermost,
channels ascending; a lane holds the same eight channels of a step in both) and end in the same fp32 epilogue -- they are bit-equal, and
that is asserted; the two weight-gradient kernels cut the position axis differently (64- and 32-row K-tiles, different splits, atomics) and
stay at the 2e-3 bar of test_conv_320_wide_kernel_at_a_chip_filling_size, the number of differing elements is printed."""
import pytest
import torch

import convnd_ref as R
from parity import close, poisoned, untouched

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _padded(t, pad, dev):
    """t [..., C] as a view into a poisoned buffer of [..., C + pad]: the pad holds NaN, which must reach no result"""
    buf = poisoned(tuple(t.shape[:-1]) + (t.shape[-1] + pad,), BF, dev)
    buf[..., :t.shape[-1]] = t.to(dev, BF)
    return buf[..., :t.shape[-1]]


def _rows(t5):
    """[N,T,H,W,C] view -> its [positions, C] row view (the position stride may exceed C)"""
    return t5.as_strided((t5.shape[0] * t5.shape[1] * t5.shape[2] * t5.shape[3], t5.shape[4]), (t5.stride(3), 1))


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _assert_bit_equal(got, want, what):
    """got (device) and want (CPU, same dtype) hold the same bits"""
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {tuple(got.shape)} {got.dtype} against {tuple(want.shape)} {want.dtype}"
    if torch.equal(_bits(got), _bits(want)):
        return
    bad = _bits(got) != _bits(want)
    at = int(bad.flatten().int().argmax())
    rows = bad.view(-1, bad.shape[-1]).any(1).nonzero().flatten()
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the reference, first at flat index {at} (got "
                         f"{got.flatten()[at].item()}, want {want.flatten()[at].item()}), in {rows.numel()} rows {rows[0].item()}..{rows[-1].item()}")


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _force_forward(dev, c, km):
    """force kernel km for the forward of case c and assert the plan the case is named after; the caller restores the setting"""
    from vt355 import ops
    ops.conv_set_tile(km, c.slots if km == 2 else 0)
    if km == 2 and c.slots == 0 and c.f320[1] > c.f320[0]:
        assert c.f320[1] > _cus(dev), f"{c.f320[1]} tiles do not exceed this device's {_cus(dev)} CUs: no workgroup would walk two tiles"
    plan = ops.conv_plan(c.N, c.T, c.H, c.W, c.Cin, c.Cout, c.k, c.pad, c.stride, c.Cin + c.pads[0], c.Cout + c.pads[1])
    want = (2,) + c.f320 if km == 2 else (1, c.f128, c.f128, 1)
    assert plan == want, f"plan (kernel, grid, tiles, tiles per workgroup) {plan}, the case is written for {want}"


def _forward(dev, c, d):
    """one forward launch of case c under the current setting -> (y view, its whole buffer)"""
    from vt355 import ops
    Ho, Wo = R.case_hw(c)
    X = _padded(d["x"], c.pads[0], dev)
    rd = None if d["res"] is None else _padded(d["res"], c.pads[2], dev)
    sb = None if d["sbias"] is None else d["sbias"].to(dev)
    ybuf = poisoned((c.N, c.T, Ho, Wo, c.Cout + c.pads[1]), BF, dev)
    y = ybuf[..., :c.Cout]
    ops.conv_cl(X, ops.pack_conv_weight_nd(d["w"]).to(dev, BF), y, c.k, c.pad, c.stride, bias=d["bias"].to(dev, BF), sbias=sb, residual=rd)
    return y, ybuf


def _force_input_grad(c, km):
    from vt355 import ops
    ops.conv_set_tile(km, 0)
    ldx = c.Cout + c.pads[3] if c.stride == 1 else c.Cout
    plan = ops.conv_plan(c.N, c.T, c.H, c.W, c.Cout, c.Cin, c.k, c.pad, 1, ldx, c.Cin + c.pads[1])
    assert plan == R.dx_plan(c, km), f"plan (kernel, grid, tiles, tiles per workgroup) {plan}, the case is written for {R.dx_plan(c, km)}"


def _input_grad(dev, c, d):
    """the input gradient as UNet.conv_bwd runs it: the stride-1 kernel with the flipped weight on dy (stride 1) or on the zero-inserted dy"""
    from vt355 import ops
    Ho, Wo = R.case_hw(c)
    dy = _padded(d["dy"], c.pads[3], dev)
    wdx = ops.pack_conv_weight_dx(d["w"]).to(dev, BF)
    dxbuf = poisoned((c.N, c.T, c.H, c.W, c.Cin + c.pads[1]), BF, dev)
    dx = dxbuf[..., :c.Cin]
    if c.stride == 1:
        ops.conv_cl(dy, wdx, dx, c.k, c.pad, 1)
    else:
        z = poisoned((c.N, c.T, c.H, c.W, c.Cout), BF, dev)
        ops.row_map(_rows(dy), z.view(-1, c.Cout), 2, c.N * c.T, Ho, Wo)
        ops.conv_cl(z, wdx, dx, c.k, c.pad, 1)
    return dx, dxbuf


def _force_weight_grad(c, km):
    from vt355 import ops
    ops.conv_set_tile(km, 0)
    plan = ops.conv_dw_plan(c.N, c.T, c.H, c.W, c.Cin, c.Cout, c.k, c.pad, c.stride, c.Cin + c.pads[0], c.Cout + c.pads[3])
    want = (2,) + c.d320 + (1, 0) if km == 2 else (1,) + c.d128 + (0, 0)
    assert plan == want, f"plan (kernel, tiles, splits, rows per split, dbias folded in, row step) {plan}, the case is written for {want}"


def _weight_grad(dev, c, d, dw, db, accumulate):
    """one weight-gradient launch into dw (+ dbias into db) under the current setting; the Linear cases go through linear_dw"""
    from vt355 import ops
    X, dy = _padded(d["x"], c.pads[0], dev), _padded(d["dy"], c.pads[3], dev)
    if c.run == "w":
        ops.linear_dw(_rows(dy), _rows(X), dw, accumulate=accumulate, dbias=db)
    else:
        ops.conv_dw_cl(dy, X, dw, c.k, c.pad, c.stride, accumulate=accumulate, dbias=db)


@pytest.mark.parametrize("name,kernel", R.fwd_pairs())
def test_exact_forward(dev, name, kernel):
    """integers and quarters: the stored bf16 must equal the fp64 reference rounded once to nearest-even, bit for bit, on either kernel"""
    from vt355 import ops
    c = R.CASES[name]
    want = R.round_bf16(R.exact_forward(name))
    try:
        _force_forward(dev, c, R.KERNELS[kernel])
        y, ybuf = _forward(dev, c, R.exact_inputs(name))
        torch.cuda.synchronize()
    finally:
        ops.conv_set_tile(0)
    _assert_bit_equal(y, want, f"{name} {kernel} forward")
    untouched(ybuf, (Ellipsis, slice(0, c.Cout)), f"{name} {kernel}: pad columns of y")


@pytest.mark.parametrize("name,kernel", R.dx_pairs())
def test_exact_input_grad(dev, name, kernel):
    from vt355 import ops
    c = R.CASES[name]
    want = R.round_bf16(R.exact_input_grad(name))
    try:
        _force_input_grad(c, R.KERNELS[kernel])
        dx, dxbuf = _input_grad(dev, c, R.exact_inputs(name))
        torch.cuda.synchronize()
    finally:
        ops.conv_set_tile(0)
    _assert_bit_equal(dx, want, f"{name} {kernel} input gradient")
    untouched(dxbuf, (Ellipsis, slice(0, c.Cin)), f"{name} {kernel}: pad columns of dx")


@pytest.mark.parametrize("name,kernel", R.dw_pairs())
def test_exact_weight_grad(dev, name, kernel):
    """a plain call into a poisoned dW and an accumulating call onto an integer pattern both give the reference exactly; the bias gradient
    (always +=) is the pattern plus the exact column sums after the first call and plus exactly twice them after the second"""
    from vt355 import ops
    c = R.CASES[name]
    d = R.exact_inputs(name)
    dwr, dbr = R.exact_weight_grad(name)
    dw1 = poisoned(tuple(dwr.shape), torch.float32, dev)
    dw2 = d["dw_fill"].to(dev)
    db = d["db_fill"].to(dev)
    try:
        _force_weight_grad(c, R.KERNELS[kernel])
        _weight_grad(dev, c, d, dw1, db, False)
        db1 = db.clone()
        _weight_grad(dev, c, d, dw2, db, True)
        torch.cuda.synchronize()
    finally:
        ops.conv_set_tile(0)
    _assert_bit_equal(dw1, dwr.float() + 0.0, f"{name} {kernel} dW")
    _assert_bit_equal(db1, (d["db_fill"].double() + dbr).float(), f"{name} {kernel} dbias")
    _assert_bit_equal(dw2, (d["dw_fill"].double() + dwr).float(), f"{name} {kernel} dW accumulated onto the pattern")
    _assert_bit_equal(db, (d["db_fill"].double() + 2 * dbr).float(), f"{name} {kernel} dbias after the second call")


@pytest.mark.parametrize("name", R.RANDN_CASES)
def test_randn_on_every_kernel(dev, name):
    """randn inputs against the fp64 reference at the bars of test_conv_cl_forward_input_grad_weight_grad on each kernel, and the kernels
    against each other (module docstring): forward and input gradient bit-equal, dW within 2e-3 of its maximum"""
    from vt355 import ops
    c = R.CASES[name]
    d = R.randn_inputs(name)
    ref, dxr, dwr, dbr = R.randn_refs(name)
    out = {}
    for kernel, km in R.KERNELS.items():
        o = {}
        try:
            if km == 1 or c.f320:
                _force_forward(dev, c, km)
                y, ybuf = _forward(dev, c, d)
                close(y, ref, 2e-2, 2e-2 * ref.abs().max().item(), f"{name} {kernel} forward")
                untouched(ybuf, (Ellipsis, slice(0, c.Cout)), f"{name} {kernel}: pad columns of y")
                o["forward"] = y.cpu()
            if dxr is not None and R.dx_plan(c, km):
                _force_input_grad(c, km)
                dx, dxbuf = _input_grad(dev, c, d)
                close(dx, dxr, 2e-2, 2e-2 * dxr.abs().max().item(), f"{name} {kernel} input gradient")
                untouched(dxbuf, (Ellipsis, slice(0, c.Cin)), f"{name} {kernel}: pad columns of dx")
                o["input gradient"] = dx.cpu()
            if km == 1 or c.d320:
                _force_weight_grad(c, km)
                dw = poisoned(tuple(dwr.shape), torch.float32, dev)
                db = torch.full((c.Cout,), 0.5, device=dev)
                _weight_grad(dev, c, d, dw, db, False)
                close(dw, dwr, 2e-2, 2e-2 * dwr.abs().max().item(), f"{name} {kernel} dW")
                close(db - 0.5, dbr, 1e-3, 2e-3 * dbr.abs().max().item(), f"{name} {kernel} dbias")
                _weight_grad(dev, c, d, dw, db, True)
                close(dw, 2 * dwr, 2e-2, 4e-2 * dwr.abs().max().item(), f"{name} {kernel} dW (accumulate)")
                close(db - 0.5, 2 * dbr, 1e-3, 4e-3 * dbr.abs().max().item(), f"{name} {kernel} dbias (accumulate)")
                o["dW"] = dw.cpu()
            torch.cuda.synchronize()
        finally:
            ops.conv_set_tile(0)
        out[kernel] = o
    for what in out["k128"]:
        if what not in out["k320"]:
            continue
        a, b = out["k128"][what], out["k320"][what]
        ndiff = int((_bits(a) != _bits(b)).sum())
        print(f"{name} {what}: {ndiff} of {a.numel()} elements differ between the kernels, max |diff| {(a.float() - b.float()).abs().max().item():.3g}")
        if what == "dW":
            assert (a - b).abs().max().item() <= 2e-3 * a.abs().max().item()
        else:
            assert ndiff == 0


def test_shape_rule_choices_for_the_real_unet(dev):
    """conv_set_tile(0): the kernels and the dW splits every convolution of the real VideoCrafter2 UNet gets at 320 x 512 x 16, one sample
    (convnd_ref.REAL_CONVS, whose list tests/test_convnd_cpu.py pins to vt355.unet.build_structure), the thresholds themselves, and the
    small cases of this file and of test_unet_kernels_gpu.py all stay on the kernels they had"""
    from vt355 import ops
    import test_unet_kernels_gpu as U
    assert _cus(dev) == 256, f"REAL_CONVS is written for the 256 CUs of an MI355X, this device has {_cus(dev)}"
    ops.conv_set_tile(0)
    assert R.real_unet_choices(ops) == R.REAL_CONVS
    # forward 320 -> 320 at 40 x 64: one sample is 320 tiles = 62.5 % of two passes (128 x 128 kernel), two are 640 = 83 % of three
    assert ops.conv_plan(1, 16, 40, 64, 320, 320) == (1, 960, 960, 1) and ops.conv_plan(2, 16, 40, 64, 320, 320) == (2, 256, 640, 3)
    assert ops.conv_plan(2, 16, 40, 64, 320, 640)[0] == 1             # 640 = 5 x 128: never by the rule
    # dW: the 320-row kernel from 2048 output positions on
    assert ops.conv_dw_plan(1, 1, 32, 64, 320, 320)[0] == 2 and ops.conv_dw_plan(1, 1, 32, 63, 320, 320)[0] == 1
    for c in R.CASES.values():
        if "f" in c.run:
            plan = ops.conv_plan(c.N, c.T, c.H, c.W, c.Cin, c.Cout, c.k, c.pad, c.stride, c.Cin + c.pads[0], c.Cout + c.pads[1])
            assert plan == (1, c.f128, c.f128, 1)
        if "w" in c.run:
            plan = ops.conv_dw_plan(c.N, c.T, c.H, c.W, c.Cin, c.Cout, c.k, c.pad, c.stride, c.Cin + c.pads[0], c.Cout + c.pads[3])
            assert plan == ((2,) + c.d320 + (1, 0) if c.d320 and R.positions(c) >= 2048 else (1,) + c.d128 + (0, 0))
    for N, T, H, W, Cin, Cout, kernel, padding, stride in U.CONV_CASES:
        Ho, Wo = R.out_hw(H, W, kernel, padding, stride)
        assert ops.conv_plan(N, T, H, W, Cin, Cout, kernel, padding, stride, Cin + 64)[0] == 1
        assert ops.conv_dw_plan(N, T, H, W, Cin, Cout, kernel, padding, stride, Cin + 64, -(-Cout // 8) * 8)[0] == (2 if Cout % 320 == 0 and N * T * Ho * Wo >= 2048 else 1)
