"""GPU parity of the VideoCrafter2 UNet kernels (csrc/convnd.hip, unet_ops.hip, attn_small.hip) through the C-ABI against
fp32 / fp64 PyTorch-CPU restatements of the same ops on the same bf16-rounded inputs."""
import math

import pytest
import torch
import torch.nn.functional as F

from parity import close, poisoned, poisoned_like, untouched, all_written

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def rb(t):
    return t.to(BF).float()


# ------------------------------------------------------------------------------------------------ convolutions
CONV_CASES = [
    # N, T, H, W, Cin, Cout, kernel, padding, stride
    (2, 2, 8, 8, 64, 128, (1, 3, 3), (0, 1, 1), 1),       # ResBlock conv 3x3
    (1, 3, 5, 7, 128, 64, (1, 3, 3), (0, 1, 1), 1),       # ragged positions
    (2, 4, 6, 5, 64, 64, (3, 1, 1), (1, 0, 0), 1),        # TemporalConvBlock (3,1,1)
    (2, 2, 8, 12, 64, 64, (1, 3, 3), (0, 1, 1), 2),       # Downsample stride 2, padding 1
    (1, 2, 6, 6, 64, 4, (1, 3, 3), (0, 1, 1), 1),         # out conv: 4 output channels
    (1, 1, 4, 4, 192, 320, (1, 1, 1), (0, 0, 0), 1),      # 1x1 skip connection, Cout not a tile multiple
    # >= 2048 output positions and Cout % 320 == 0: the weight gradient takes the 320-row loader / multiplier kernel (conv_dw320_kernel)
    (1, 4, 16, 32, 320, 320, (1, 3, 3), (0, 1, 1), 1),    # ResBlock 3x3 at the UNet's first width
    (2, 8, 12, 16, 64, 320, (3, 1, 1), (1, 0, 0), 1),     # temporal taps; (tap, ci) axis 192 wide: the second 128-column tile is half empty
    (1, 2, 64, 48, 64, 320, (1, 3, 3), (0, 1, 1), 1),     # the input convolution (4 -> 320, channels padded to 64): 576 columns = 4.5 tiles
    (1, 4, 48, 48, 64, 640, (1, 3, 3), (0, 1, 1), 2),     # stride 2, two 320-row blocks
    (1, 3, 30, 25, 64, 320, (1, 3, 3), (0, 1, 1), 1),     # 2250 positions: ragged last K-tile, ragged position split
]


def _conv_ref(x, w, b, kernel, padding, stride):
    """x [N,T,H,W,Cin] fp32 -> [N,T,Ho,Wo,Cout] with torch's conv3d (Conv2d == one temporal tap)"""
    xi = x.permute(0, 4, 1, 2, 3)
    w5 = w if w.dim() == 5 else w[:, :, None]
    y = F.conv3d(xi, w5, b, stride=(1, stride, stride), padding=padding)
    return y.permute(0, 2, 3, 4, 1)


@pytest.mark.parametrize("N,T,H,W,Cin,Cout,kernel,padding,stride", CONV_CASES)
def test_conv_cl_forward_input_grad_weight_grad(dev, N, T, H, W, Cin, Cout, kernel, padding, stride):
    from vt355 import ops
    g = torch.Generator().manual_seed(H * W + Cout + Cin)
    KT, KH, KW = kernel
    x = rb(torch.randn(N, T, H, W, Cin, generator=g))
    wshape = (Cout, Cin, KH, KW) if KT == 1 else (Cout, Cin, KT, KH, KW)
    w = rb(torch.randn(wshape, generator=g) / math.sqrt(Cin * KT * KH * KW))
    b = rb(torch.randn(Cout, generator=g) * 0.1)
    sb = torch.randn(N, Cout, generator=g) * 0.1
    xr = x.clone().requires_grad_(True); wr = w.clone().requires_grad_(True)
    ref = _conv_ref(xr, wr, b, kernel, padding, stride) + sb[:, None, None, None, :]
    res = rb(torch.randn(ref.shape, generator=g))
    dy = rb(torch.randn(ref.shape, generator=g))
    (ref * dy).sum().backward()
    Ho, Wo = ref.shape[2], ref.shape[3]
    # ---- forward (+ bias, per-sample bias, residual), input slice of a wider buffer ----
    xb = torch.zeros(N, T, H, W, Cin + 64, dtype=BF, device=dev)
    xb[..., :Cin] = x.to(dev, BF)
    y = poisoned((N, T, Ho, Wo, Cout), BF, dev)
    ops.conv_cl(xb[..., :Cin], ops.pack_conv_weight_nd(w).to(dev, BF), y, kernel, padding, stride, bias=b.to(dev, BF), sbias=sb.to(dev),
                residual=res.to(dev, BF))
    close(y, ref.detach() + res, 2e-2, 2e-2 * ref.abs().max().item(), "conv forward")
    # ---- weight gradient ----
    dw = poisoned((Cout, KT * KH * KW * Cin), torch.float32, dev)           # accumulate=False writes it whole; the second call adds to it
    dyd = torch.zeros(N, T, Ho, Wo, (Cout + 7) // 8 * 8, dtype=BF, device=dev)[..., :Cout]       # rows are 16-byte multiples
    dyd.copy_(dy.to(dev, BF))
    db = torch.full((Cout,), 0.5, device=dev)                  # the bias gradient rides along (+=): column sums of dy
    ops.conv_dw_cl(dyd, xb[..., :Cin], dw, kernel, padding, stride, accumulate=False, dbias=db)
    dwr = ops.pack_conv_weight_nd(wr.grad)
    close(dw, dwr, 2e-2, 2e-2 * dwr.abs().max().item(), "conv weight gradient")
    dbr = dy.double().sum((0, 1, 2, 3)).float()
    close(db - 0.5, dbr, 1e-3, 2e-3 * dbr.abs().max().item(), "conv bias gradient")
    ops.conv_dw_cl(dyd, xb[..., :Cin], dw, kernel, padding, stride, accumulate=True, dbias=db)
    close(dw, 2 * dwr, 2e-2, 4e-2 * dwr.abs().max().item(), "conv weight gradient (accumulate)")
    close(db - 0.5, 2 * dbr, 1e-3, 4e-3 * dbr.abs().max().item(), "conv bias gradient (accumulate)")
    # ---- input gradient: the same kernel with the flipped, transposed weight (stride 1) / on the zero-inserted dy (stride 2) ----
    if Cout % 64:
        return
    wdx = ops.pack_conv_weight_dx(w if w.dim() == 5 else w[:, :, None]).to(dev, BF)
    dx = poisoned((N, T, H, W, Cin), BF, dev)
    if stride == 1:
        ops.conv_cl(dy.to(dev, BF), wdx, dx, kernel, padding, 1)
    else:
        z = poisoned((N, T, H, W, Cout), BF, dev)
        ops.row_map(dy.to(dev, BF).view(-1, Cout), z.view(-1, Cout), 2, N * T, Ho, Wo)
        ops.conv_cl(z, wdx, dx, kernel, padding, 1)
    close(dx, xr.grad, 2e-2, 2e-2 * xr.grad.abs().max().item(), "conv input gradient")


@pytest.mark.parametrize("N,T,H,W,Cin,Cout,kernel,padding,stride", [c for c in CONV_CASES if c[5] % 320 == 0 and c[4] % 64 == 0])
def test_conv_320_wide_kernels_forced(dev, N, T, H, W, Cin, Cout, kernel, padding, stride):
    """the 128 x 320 forward / input-gradient kernel (convnd320_kernel) picks itself only when its tiles fill the chip (>= 32 768 positions
    at 320 channels); here it and the 320-row weight-gradient kernel are FORCED (vt_conv_set_tile(2)) onto the small cases -- ragged
    position tiles, stride 2, temporal taps, two channel blocks -- and must agree with the reference exactly as the 128 x 128 kernels do"""
    from vt355 import ops
    ops.conv_set_tile(2)
    try:
        test_conv_cl_forward_input_grad_weight_grad(dev, N, T, H, W, Cin, Cout, kernel, padding, stride)
    finally:
        ops.conv_set_tile(0)


def test_conv_320_wide_kernel_at_a_chip_filling_size(dev):
    """[1, 16, 40, 64] x 320 -> 320, 3x3 (one sample of the UNet's first level: 40 960 positions = 320 tiles of 128 x 320): the kernel choice is
    the library's own here; the 128 x 128 kernels (vt_conv_set_tile(1)) on the same inputs are the comparison (both are pinned to the fp32
    reference by the small cases above)"""
    from vt355 import ops
    g = torch.Generator().manual_seed(11)
    N, T, H, W, C = 1, 16, 40, 64, 320
    x = rb(torch.randn(N, T, H, W, C, generator=g)).to(dev, BF)
    w = rb(torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C))
    wk = ops.pack_conv_weight_nd(w).to(dev, BF)
    b = rb(torch.randn(C, generator=g) * 0.1).to(dev, BF)
    sb = (torch.randn(N, C, generator=g) * 0.1).to(dev)
    res = rb(torch.randn(N, T, H, W, C, generator=g)).to(dev, BF)
    dy = rb(torch.randn(N, T, H, W, C, generator=g)).to(dev, BF)
    out = {}
    for mode in (1, 0):
        ops.conv_set_tile(mode)
        try:
            y = poisoned((N, T, H, W, C), BF, dev)
            ops.conv_cl(x, wk, y, (1, 3, 3), (0, 1, 1), 1, bias=b, sbias=sb, residual=res)
            dw = poisoned((C, 9 * C), torch.float32, dev)
            ops.conv_dw_cl(dy, x, dw, (1, 3, 3), (0, 1, 1), 1, accumulate=False)
            out[mode] = (y.float(), dw.clone())
        finally:
            ops.conv_set_tile(0)
    torch.cuda.synchronize()
    y1, dw1 = out[1]; y0, dw0 = out[0]
    assert torch.isfinite(y0).all() and torch.isfinite(dw0).all()
    assert (y0 - y1).abs().max().item() <= 2.0 ** -6 * y1.abs().max().item()              # same products, same fp32 sums up to order: one bf16 ulp
    assert (dw0 - dw1).abs().max().item() <= 2e-3 * dw1.abs().max().item()


def _extents(ldx, lddy, N, T, H, W, Cin, Cout, kernel, padding, stride):
    import ctypes as C
    from vt355._lib import load_library, check
    a, b, c = C.c_longlong(), C.c_longlong(), C.c_longlong()
    check(load_library().vt_conv_desc_extents(ldx, lddy, N, T, H, W, Cin, Cout, kernel[1], kernel[2], padding[1], padding[2], stride,
                                              C.byref(a), C.byref(b), C.byref(c)), "vt_conv_desc_extents")
    return a.value, b.value, c.value


@pytest.mark.parametrize("N,T,H,W,C1,Cin,Cout,kernel,padding", [
    (1, 2, 8, 16, 320, 320, 320, (1, 3, 3), (0, 1, 1)),       # the geometry of gpurun_out/r2_vc2_b1.log: skip concat 320 | 320, ragged 128-column tiles
    (2, 2, 8, 8, 64, 192, 320, (1, 3, 3), (0, 1, 1)),         # unequal halves, Cin not a tile multiple either
    (1, 4, 4, 8, 128, 64, 64, (3, 1, 1), (1, 0, 0)),          # the temporal (3,1,1) convolution on a trailing slice
    (1, 4, 16, 32, 320, 320, 320, (1, 3, 3), (0, 1, 1)),      # 2048 positions: the 320-row weight-gradient kernel on trailing slices
])
def test_conv_on_trailing_column_slices_stays_inside_the_allocation(dev, N, T, H, W, C1, Cin, Cout, kernel, padding):
    """Regression test of the round-2 memory access fault (first full-size VC2 backward): the gradient of the SECOND half of a skip
    concatenation (openaimodel3d.py:686-690) is a TRAILING column slice `buf[..., C1:]`; `rows * ld` counted from that base lies C1 columns
    past the end of the allocation, and a ragged last column tile of the last rows read there.  The descriptors must end with the last
    row's logical columns: asserted on the extents the library reports BEFORE anything is launched, then the kernels run on buffers that
    end exactly at their allocation (a fresh hipMalloc, 2 MiB granules) and are compared with the fp32 reference."""
    from vt355 import ops
    g = torch.Generator().manual_seed(C1 + Cin + Cout)
    KT, KH, KW = kernel
    Ho, Wo = H, W
    x = rb(torch.randn(N, T, H, W, Cin, generator=g))
    dy = rb(torch.randn(N, T, Ho, Wo, Cout, generator=g))
    wshape = (Cout, Cin, KH, KW) if KT == 1 else (Cout, Cin, KT, KH, KW)
    w = rb(torch.randn(wshape, generator=g) / math.sqrt(Cin * KT * KH * KW))
    torch.cuda.empty_cache()                      # the next allocations come straight from hipMalloc: the slices end where their mapping ends
    xbuf = torch.zeros(N, T, H, W, C1 + Cin, dtype=BF, device=dev)
    dybuf = torch.zeros(N, T, Ho, Wo, C1 + Cout, dtype=BF, device=dev)
    xs, dys = xbuf[..., C1:], dybuf[..., C1:]         # trailing slices: base = allocation base + C1 columns
    xs.copy_(x.to(dev, BF)); dys.copy_(dy.to(dev, BF))
    fwd_x, dw_x, dw_dy = _extents(xs.stride(3), dys.stride(3), N, T, H, W, Cin, Cout, kernel, padding, 1)
    room_x = (xbuf.numel() - C1) * 2                  # bytes from the slice base to the end of the allocation
    room_dy = (dybuf.numel() - C1) * 2
    assert fwd_x <= room_x and dw_x <= room_x, (fwd_x, dw_x, room_x)
    assert dw_dy <= room_dy, (dw_dy, room_dy)
    assert fwd_x == room_x and dw_dy == room_dy       # and not a byte less: the last row is read whole
    # the input-gradient convolution reads dy (a trailing slice) as ITS x: same descriptor rule
    dx_x, _, _ = _extents(dys.stride(3), xs.stride(3), N, T, Ho, Wo, Cout, Cin, kernel, padding, 1)
    assert dx_x <= room_dy
    xr = x.clone().requires_grad_(True); wr = w.clone().requires_grad_(True)
    ref = _conv_ref(xr, wr, None, kernel, padding, 1)
    (ref * dy).sum().backward()
    y = poisoned((N, T, Ho, Wo, Cout), BF, dev)
    ops.conv_cl(xs, ops.pack_conv_weight_nd(w).to(dev, BF), y, kernel, padding, 1)
    close(y, ref.detach(), 2e-2, 2e-2 * ref.abs().max().item(), "conv forward on a trailing slice")
    dw = poisoned((Cout, KT * KH * KW * Cin), torch.float32, dev)
    ops.conv_dw_cl(dys, xs, dw, kernel, padding, 1, accumulate=False)
    dwr = ops.pack_conv_weight_nd(wr.grad)
    close(dw, dwr, 2e-2, 2e-2 * dwr.abs().max().item(), "conv weight gradient, dy and x trailing slices")
    wdx = ops.pack_conv_weight_dx(w if w.dim() == 5 else w[:, :, None]).to(dev, BF)
    dx = poisoned((N, T, H, W, Cin), BF, dev)
    ops.conv_cl(dys, wdx, dx, kernel, padding, 1)
    close(dx, xr.grad, 2e-2, 2e-2 * xr.grad.abs().max().item(), "conv input gradient from a trailing dy slice")
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,P,Q", [(1000, 320, 320), (77, 64, 1024), (4096, 2560, 320), (300, 8, 72)])
def test_linear_dw_any_size(dev, M, P, Q):
    from vt355 import ops
    g = torch.Generator().manual_seed(M + P)
    dy = rb(torch.randn(M, P, generator=g)); x = rb(torch.randn(M, Q, generator=g))
    ref = dy.double().t() @ x.double()
    dw = poisoned((P, Q), torch.float32, dev)
    ops.linear_dw(dy.to(dev, BF), x.to(dev, BF), dw, accumulate=False)
    close(dw, ref, 1e-2, 1e-2 * ref.abs().max().item(), "linear dW")


def test_weight_gradients_over_rows_spanning_more_than_2_gib(dev):
    """vt_conv_dw_bias_cl (one tap) and vt_gemm_nt_bf16 sum over token rows; one buffer descriptor covers < 2 GiB, so the entry points walk
    longer row ranges in chunks (HunyuanVideo's 720p x 129-frame sequence on one card: 119 312 rows x 21 504 columns = 5 GB).  Here: 700
    rows 5 MB apart (3.5 GB span, three chunks), against fp64 and against the same rows stored compactly."""
    from vt355 import ops
    M, P, Q, W = 700, 256, 384, 2_500_000
    g = torch.Generator().manual_seed(11)
    dy = rb(torch.randn(M, P, generator=g)); x = rb(torch.randn(M, Q, generator=g))
    ref = dy.double().t() @ x.double()
    wide = poisoned((M, W), BF, dev)             # input staging: only the two column slices filled below may be read
    assert M * W * 2 > 2 ** 31 + 2 ** 30
    wide[:, :P] = dy.to(dev, BF); wide[:, 1024:1024 + Q] = x.to(dev, BF)
    dyw, xw = wide[:, :P], wide[:, 1024:1024 + Q]
    tol = 1e-2 * ref.abs().max().item()
    dw = poisoned((P, Q), torch.float32, dev); db = torch.zeros(P, device=dev)       # db is in/out: the bias gradient accumulates
    ops.linear_dw(dyw, xw, dw, accumulate=False, dbias=db)
    close(dw, ref, 1e-2, tol, "chunked linear dW")
    close(db, dy.double().sum(0), 1e-2, 1e-2 * M ** 0.5, "chunked bias gradient")
    ops.linear_dw(dyw, xw, dw, accumulate=True)
    close(dw, 2 * ref, 1e-2, 2 * tol, "chunked linear dW, accumulated")
    c = poisoned((P, Q), torch.float32, dev)
    ops.gemm_nt(dyw, xw, c, accumulate=False)
    close(c, ref, 1e-2, tol, "chunked gemm_nt")
    ops.gemm_nt(dyw, xw, c, alpha=0.5, accumulate=True)
    close(c, 1.5 * ref, 1e-2, 2 * tol, "chunked gemm_nt, accumulated")
    c2 = poisoned((P, Q), torch.float32, dev)
    ops.gemm_nt(dy.to(dev, BF), x.to(dev, BF), c2, accumulate=False)
    close(c2, ref, 1e-2, tol, "compact gemm_nt")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("M,C,ld,p,seed,off", [(1000, 320, 320, 0.1, 12345, 0), (77, 64, 128, 0.1, 2 ** 40 + 3, 7 << 36), (512, 1280, 1280, 0.5, 9, 1 << 36)])
def test_dropout_mask_is_philox_and_backward_reuses_it(dev, M, C, ld, p, seed, off):
    """vt_dropout_bf16: the keep mask equals oracle/philox.py's Philox4x32-10 restatement bit for bit (Random123 known answers pin that
    on the CPU), kept values are x / (1 - p) rounded to bf16, and the same (seed, offset) on a second tensor (the gradient) gives the
    same mask -- nothing is stored between forward and backward"""
    import philox
    from vt355 import ops
    g = torch.Generator().manual_seed(M + C)
    x = rb(torch.randn(M, C, generator=g))
    xb = torch.zeros(M, ld, dtype=BF, device=dev)[:, :C]
    xb.copy_(x.to(dev, BF))
    y = poisoned((M, C), BF, dev)
    mask = poisoned((M, C), torch.uint8, dev)
    ops.dropout(xb, y, p, seed, off, mask_out=mask)
    want = torch.from_numpy(philox.dropout_keep_mask(M, C, p, seed, off))
    all_written(mask, "dropout keep mask")
    assert torch.equal(mask.cpu(), want)
    ref = (x * want.float() / (1.0 - p)).to(BF).float()
    assert torch.equal(y.float().cpu(), ref)
    dy = rb(torch.randn(M, C, generator=g))
    dx = poisoned((M, C), BF, dev)
    ops.dropout(dy.to(dev, BF), dx, p, seed, off)
    assert torch.equal(dx.float().cpu(), (dy * want.float() / (1.0 - p)).to(BF).float())
    assert abs(want.float().mean().item() - (1 - p)) < 0.02


# ------------------------------------------------------------------------------------------------ GroupNorm backward
@pytest.mark.parametrize("N,P,C,silu,eps", [(2, 50, 64, True, 1e-5), (3, 33, 320, True, 1e-5), (2, 64, 128, False, 1e-6), (1, 20, 2560, True, 1e-5)])
def test_groupnorm_forward_backward(dev, N, P, C, silu, eps):
    from vt355 import ops
    g = torch.Generator().manual_seed(C + P)
    x = rb(torch.randn(N, P, C, generator=g) * 1.5 + 0.3)
    ga = rb(1 + 0.2 * torch.randn(C, generator=g)); be = rb(0.2 * torch.randn(C, generator=g))
    dy = rb(torch.randn(N, P, C, generator=g))
    xr = x.clone().double().requires_grad_(True); gr = ga.double().requires_grad_(True); br = be.double().requires_grad_(True)
    y = F.group_norm(xr.permute(0, 2, 1), 32, gr, br, eps).permute(0, 2, 1)
    if silu:
        y = F.silu(y)
    (y * dy.double()).sum().backward()
    xd = x.to(dev, BF); yd = poisoned_like(xd)
    ws = ops.groupnorm_fwd(xd, ga.to(dev, BF), be.to(dev, BF), yd, 32, eps, silu)
    close(yd, y, 2e-2, 2e-2, "groupnorm forward")
    dx = poisoned_like(xd)
    dga = torch.zeros(C, device=dev); dbe = torch.zeros(C, device=dev)          # in/out: the parameter gradients accumulate
    ops.groupnorm_bwd(dy.to(dev, BF), xd, ga.to(dev, BF), ws, dx, dga, dbe, 32, silu)
    close(dx, xr.grad, 3e-2, 2e-2 * xr.grad.abs().max().item(), "groupnorm dx")
    close(dga, gr.grad, 2e-2, 2e-2 * gr.grad.abs().max().item(), "groupnorm dgamma")
    close(dbe, br.grad, 2e-2, 2e-2 * br.grad.abs().max().item(), "groupnorm dbeta")
    base = rb(torch.randn(N, P, C, generator=g))
    dx2 = base.to(dev, BF).clone()
    ops.groupnorm_bwd(dy.to(dev, BF), xd, ga.to(dev, BF), ws, dx2, None, None, 32, silu, accumulate=True)
    close(dx2, xr.grad + base, 3e-2, 3e-2 * xr.grad.abs().max().item(), "groupnorm dx (accumulate)")


# ------------------------------------------------------------------------------------------------ GEGLU, row maps, loss
def test_geglu_forward_backward(dev):
    from vt355 import ops
    g = torch.Generator().manual_seed(3)
    M, Fd = 77, 320
    h = rb(torch.randn(M, 2 * Fd, generator=g) * 2); dy = rb(torch.randn(M, Fd, generator=g))
    hr = h.clone().double().requires_grad_(True)
    a, gate = hr.chunk(2, dim=-1)
    y = a * F.gelu(gate)
    (y * dy.double()).sum().backward()
    yd = poisoned((M, Fd), BF, dev)
    ops.geglu_fwd(h.to(dev, BF), yd)
    close(yd, y, 1e-2, 1e-2, "geglu")
    dh = poisoned((M, 2 * Fd), BF, dev)
    ops.geglu_bwd(dy.to(dev, BF), h.to(dev, BF), dh)
    close(dh, hr.grad, 1e-2, 2e-2, "geglu backward")


def test_row_maps_add_and_loss(dev):
    from vt355 import ops
    g = torch.Generator().manual_seed(4)
    B, T, HW, C = 2, 4, 6, 64
    x = rb(torch.randn(B, T, HW, C, generator=g))
    xd = x.to(dev, BF).view(-1, C)
    out = poisoned((B * HW * T, C), BF, dev)
    ops.row_map(xd, out, 0, B, T, HW)
    assert torch.equal(out.float().cpu().view(B, HW, T, C), x.permute(0, 2, 1, 3))
    back = poisoned_like(xd)
    ops.row_map(out, back, 0, B, HW, T)
    assert torch.equal(back, xd)
    N, H, W = 3, 2, 3
    s = rb(torch.randn(N, H, W, C, generator=g))
    up = poisoned((N * 4 * H * W, C), BF, dev)
    ops.row_map(s.to(dev, BF).view(-1, C), up, 1, N, H, W)
    ref = s.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    assert torch.equal(up.float().cpu().view(N, 2 * H, 2 * W, C), ref)
    up = poisoned((N * 4 * H * W, C), BF, dev)      # fresh: mode 1 left the same values at the even positions
    ops.row_map(s.to(dev, BF).view(-1, C), up, 2, N, H, W)
    z = torch.zeros(N, 2 * H, 2 * W, C); z[:, ::2, ::2] = s
    assert torch.equal(up.float().cpu().view(N, 2 * H, 2 * W, C), z)
    big = rb(torch.randn(N, 2 * H, 2 * W, C, generator=g))
    dn = poisoned((N * H * W, C), BF, dev)
    ops.row_map(big.to(dev, BF).view(-1, C), dn, 3, N, H, W)
    close(dn.view(N, H, W, C), big.view(N, H, 2, W, 2, C).sum(dim=(2, 4)), 1e-2, 1e-2, "2x2 block sum")
    ops.row_map(big.to(dev, BF).view(-1, C), dn, 3, N, H, W, accumulate=True)
    close(dn.view(N, H, W, C), 2 * big.view(N, H, 2, W, 2, C).sum(dim=(2, 4)), 1e-2, 2e-2, "2x2 block sum (accumulate)")
    a = rb(torch.randn(10, C, generator=g)); b = rb(torch.randn(10, C, generator=g))
    o = poisoned((10, C), BF, dev)
    ops.add_rows(a.to(dev, BF), b.to(dev, BF), o)
    close(o, a + b, 1e-2, 1e-2, "add rows")
    # q_sample + eps-MSE loss
    x0 = torch.randn(2, 4, 4, 8, 8, generator=g); nz = torch.randn(x0.shape, generator=g)
    sa = torch.tensor([0.9, 0.3]); sb = torch.tensor([0.4, 0.95]); sc = torch.tensor([1.0, 0.7])
    xt = poisoned(x0.shape, BF, dev)
    ops.q_sample(x0.to(dev), nz.to(dev), sa.to(dev), sb.to(dev), sc.to(dev), xt)
    close(xt, (sa * sc).view(2, 1, 1, 1, 1) * x0 + sb.view(2, 1, 1, 1, 1) * nz, 1e-2, 1e-2, "q_sample")
    pred = rb(torch.randn(x0.shape, generator=g))
    loss = poisoned((1,), torch.float32, dev); dp = poisoned(x0.shape, BF, dev)
    ops.mse_loss(pred.to(dev, BF), nz.to(dev), loss, dp, grad_scale=0.5)
    ref = ((pred - nz) ** 2).mean(dim=(1, 2, 3, 4)).mean()
    assert abs(loss.item() - ref.item()) < 1e-4 * ref.item()
    close(dp, 0.5 * 2 * (pred - nz) / pred.numel(), 1e-2, 1e-6, "mse gradient")


# ------------------------------------------------------------------------------------------------ short-key attention
def _attn_ref(q, k, v, scale, mask_block=0):
    """q [NB,H,Sq,64], k/v [NB,H,Sk,64] float64"""
    s = torch.einsum("bhid,bhjd->bhij", q, k) * scale
    if mask_block:
        i = torch.arange(q.shape[2])[:, None] // mask_block
        j = torch.arange(k.shape[2])[None, :] // mask_block
        s = s.masked_fill(i != j, float("-inf"))
    return torch.einsum("bhij,bhjd->bhid", s.softmax(-1), v)


def _zero_ref_scale(r, dv_ref):
    """the absolute tolerance of a gradient scales with max |reference|.  With ONE key per query the softmax is the constant 1 and the
    references of dq and dk are identically zero, while the device's dS = p (dO . v - dO . o) keeps the bf16 rounding of o: an error
    relative to |dO| |v|, which is the scale of dv = p^T dO -- so a gradient whose own reference is zero is held to max |dv_ref|"""
    return r.abs().max().item() or dv_ref.abs().max().item()


@pytest.mark.parametrize("NB,H,Sq,Sk", [(2, 2, 300, 77), (1, 5, 1500, 77), (3, 1, 40, 20), (1, 2, 130, 128),
                                        (2, 2, 130, 33), (1, 1, 129, 64), (1, 2, 1025, 96), (1, 1, 1, 1)])
def test_attn_small_cross(dev, NB, H, Sq, Sk):
    """text cross-attention (CrossAttention.forward, lvdm/modules/attention.py:101-181): every query of a sample against its <= 128 keys.
    One, two (33 and 64 keys), three and four 32-key tiles; 1025 queries cross the backward's 1024-query chunk with a one-row tail; a
    single query against a single key.  o, lse and dq are written whole, dk / dv are fp32 accumulators the binding zeroes"""
    from vt355 import ops
    g = torch.Generator().manual_seed(Sq + Sk)
    D = H * 64
    q = rb(torch.randn(NB, Sq, D, generator=g)); kv = rb(torch.randn(NB, Sk, 2 * D, generator=g))
    do = rb(torch.randn(NB, Sq, D, generator=g))
    sp = lambda t: t.double().view(t.shape[0], t.shape[1], H, 64).permute(0, 2, 1, 3)
    qr, kr, vr = sp(q).requires_grad_(True), sp(kv[..., :D]).requires_grad_(True), sp(kv[..., D:]).requires_grad_(True)
    ref = _attn_ref(qr, kr, vr, 0.125)
    (ref * sp(do)).sum().backward()
    mg = lambda t: t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], D)
    qd, kvd = q.to(dev, BF), kv.to(dev, BF)
    o = poisoned((NB, Sq, D), BF, dev); lse = poisoned((NB, H, Sq), torch.float32, dev)
    ops.attn_small_fwd(qd, kvd[..., :D], kvd[..., D:], o, lse, H, 0.125)
    close(o, mg(ref), 2e-2, 1e-2, "cross-attention output")
    dq = poisoned((NB, Sq, D), BF, dev)
    dk = poisoned((NB, Sk, D), torch.float32, dev); dv = poisoned((NB, Sk, D), torch.float32, dev)
    ops.attn_small_bwd(qd, kvd[..., :D], kvd[..., D:], o, do.to(dev, BF), lse, dq, dk, dv, H, 0.125)
    for got, r, nm in ((dq, qr.grad, "dq"), (dk, kr.grad, "dk"), (dv, vr.grad, "dv")):
        close(got, mg(r), 3e-2, 2e-2 * _zero_ref_scale(r, vr.grad), "cross-attention " + nm)
    lref = torch.logsumexp(torch.einsum("bhid,bhjd->bhij", qr, kr).detach() * 0.125, -1) * 1.4426950408889634
    close(lse, lref, 1e-3, 2e-2, "cross-attention lse2")


def test_attn_small_refuses_more_than_128_keys_and_odd_sequence_lengths(dev):
    """129 keys do not fit the resident key set; a packed sequence length must divide the 32-row tile (T = 3 does not): both are refused
    on the host, forward and backward, and the library writes nothing (the binding zeroes the cross form's fp32 dk / dv accumulators before
    it calls the library: those come back as zeros)"""
    from vt355 import ops
    from vt355._lib import VtError
    D = 64
    for Sq, Sk, T in ((40, 129, 0), (96, 96, 3)):
        NB = 1
        q = torch.zeros(NB, Sq, D, dtype=BF, device=dev); kv = torch.zeros(NB, Sk, 2 * D, dtype=BF, device=dev)
        o = poisoned((NB, Sq, D), BF, dev); lse = poisoned((NB, 1, Sq), torch.float32, dev)
        dq = poisoned((NB, Sq, D), BF, dev)
        dk, dv = (poisoned((NB, Sk, D), BF, dev) for _ in range(2)) if T else (poisoned((NB, Sk, D), torch.float32, dev) for _ in range(2))
        with pytest.raises(VtError, match="vt_attn_small_fwd"):
            ops.attn_small_fwd(q, kv[..., :D], kv[..., D:], o, lse, 1, 0.125, mask_block=T)
        with pytest.raises(VtError, match="vt_attn_small_bwd"):
            ops.attn_small_bwd(q, kv[..., :D], kv[..., D:], q, q, torch.zeros_like(lse), dq, dk, dv, 1, 0.125, mask_block=T)
        untouched(o, [], "refused attn_small_fwd: o"); untouched(lse, [], "refused attn_small_fwd: lse"); untouched(dq, [], "refused attn_small_bwd: dq")
        if T:                                # bf16 dk / dv belong to the kernel alone: nothing is written
            untouched(dk, [], "refused attn_small_bwd: dk"); untouched(dv, [], "refused attn_small_bwd: dv")
        else:                                # the fp32 accumulators are zeroed by the binding before the library refuses: zeros, and nothing added
            assert bool((dk == 0).all()) and bool((dv == 0).all()), "refused attn_small_bwd: dk / dv accumulators"


@pytest.mark.parametrize("R,T,H", [(256, 16, 2), (80, 16, 1), (40960, 16, 5), (72, 4, 8), (33 * 8, 8, 1), (160, 32, 2), (130, 2, 1), (97, 1, 2)])
def test_attn_small_packed_sequences(dev, R, T, H):
    """temporal self-attention (TemporalTransformer, attention.py:395-519): R / T consecutive sequences of T rows, fused qkv.  Every divisor
    of the 32-row tile is a legal T: 32 (a 128-row item plus a 32-row tail), 16, 8, 4, 2 (a two-row tail item) and 1.  At T = 1 the one
    unmasked probability is exp2(0) = 1, so by the kernel's own arithmetic o == v and dv == dO bit for bit"""
    from vt355 import ops
    g = torch.Generator().manual_seed(R + T)
    D = H * 64
    big = R > 5000
    qkv = rb(torch.randn(R, 3 * D, generator=g))
    do = rb(torch.randn(R, D, generator=g))
    d = qkv.to(dev, BF).view(1, R, 3 * D)
    o = poisoned((1, R, D), BF, dev); lse = poisoned((1, H, R), torch.float32, dev)
    ops.attn_small_fwd(d[..., :D], d[..., D:2 * D], d[..., 2 * D:], o, lse, H, 0.125, mask_block=T)
    dqkv = poisoned((1, R, 3 * D), BF, dev)
    ops.attn_small_bwd(d[..., :D], d[..., D:2 * D], d[..., 2 * D:], o, do.to(dev, BF).view(1, R, D), lse,
                       dqkv[..., :D], dqkv[..., D:2 * D], dqkv[..., 2 * D:], H, 0.125, mask_block=T)
    rows = slice(R - 2048, R) if big else slice(0, R)          # the full first-level size: check the last 128 sequences
    n = (rows.stop - rows.start) // T
    x = qkv[rows].double().view(n, T, 3, H, 64).permute(2, 0, 3, 1, 4).clone().requires_grad_(True)   # [3, n, H, T, 64]
    ref = _attn_ref(x[0], x[1], x[2], 0.125)
    (ref * do[rows].double().view(n, T, H, 64).permute(0, 2, 1, 3)).sum().backward()
    close(o[0, rows], ref.permute(0, 2, 1, 3).reshape(n * T, D), 2e-2, 1e-2, "temporal attention output")
    gref = x.grad.permute(1, 3, 0, 2, 4).reshape(n * T, 3 * D)
    if T == 1:
        assert torch.equal(o[0], d[0, :, 2 * D:]), "T = 1: o must equal v bit for bit"
        assert torch.equal(dqkv[0, :, 2 * D:], do.to(dev, BF)), "T = 1: dv must equal dO bit for bit"
        assert gref[:, :2 * D].abs().max().item() == 0.0                # the references of dq and dk are identically zero: _zero_ref_scale
        close(dqkv[0, :, :2 * D], gref[:, :2 * D], 3e-2, 2e-2 * gref[:, 2 * D:].abs().max().item(), "temporal attention dq | dk at T = 1")
    else:
        close(dqkv[0, rows], gref, 3e-2, 2e-2 * gref.abs().max().item(), "temporal attention dqkv")
    if big:                                                             # written whole: the rows not compared above are at least finite
        assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(dqkv.float()).all()) and bool(torch.isfinite(lse).all())


# ------------------------------------------------------------------------------------------------ generic-head-dim attention
def _gen_case(dev, NB, H, Sq, Sk, hd, hstride, kv_len=None, mask_block=0, seed=0, bf16_out=False, shape_keys=None):
    """every output is poisoned first.  Written whole: the head_dim (80 | 128) columns of every head of o and dq, lse, dk / dv in the packed
    and the bf16 forms (the fp32 dk / dv accumulators are zeroed by the binding and summed into).  Never written: the columns between
    head_dim and hstride of every head.  bf16 dk / dv rows at and past a sample's kv_len come back exactly 0.
    shape_keys: applied to the randn keys [NB, Sk, H, hstride] in place before they are rounded to bf16 (tests/test_conditioning_gpu.py)."""
    from vt355 import ops
    g = torch.Generator().manual_seed(seed + Sq + Sk + hd)
    hp = 80 if hd == 72 else 128
    def mk(S, shape=None):
        t = torch.zeros(NB, S, H, hstride)
        t[..., :hd] = torch.randn(NB, S, H, hd, generator=g)
        if shape is not None:
            shape(t)
        return rb(t)
    q, k, v, do = mk(Sq), mk(Sk, shape_keys), mk(Sk), mk(Sq)
    scale = hd ** -0.5
    qr, kr, vr = [t[..., :hd].double().permute(0, 2, 1, 3).clone().requires_grad_(True) for t in (q, k, v)]
    s = torch.einsum("bhid,bhjd->bhij", qr, kr) * scale
    if kv_len is not None:
        for b, n in enumerate(kv_len):
            s[b, :, :, n:] = float("-inf")
    if mask_block:
        i = torch.arange(Sq)[:, None] // mask_block; j = torch.arange(Sk)[None, :] // mask_block
        s = s.masked_fill(i != j, float("-inf"))
    ref = torch.einsum("bhij,bhjd->bhid", s.softmax(-1), vr)
    (ref * do[..., :hd].double().permute(0, 2, 1, 3)).sum().backward()
    D = H * hstride
    fl = lambda t: t.reshape(NB, -1, D).to(dev, BF)
    qd, kd, vd, dod = fl(q), fl(k), fl(v), fl(do)
    o = poisoned((NB, Sq, D), BF, dev); lse = poisoned((NB, H, Sq), torch.float32, dev)
    kl = None if kv_len is None else torch.tensor(kv_len, dtype=torch.int32, device=dev)
    ops.attn_gen_fwd(qd, kd, vd, o, lse, H, hp, hstride, scale, kv_len=kl, mask_block=mask_block)
    un = lambda t: t.view(NB, -1, H, hstride)[..., :hd].permute(0, 2, 1, 3)
    close(un(o), ref, 2e-2, 1e-2, "attention output")
    stored = lambda t: (slice(None), slice(None), slice(None), slice(0, hp))        # of the [NB, S, H, hstride] view
    untouched(o.view(NB, Sq, H, hstride), stored(o), "attention output: columns past head_dim")
    assert bool(torch.isfinite(o.float().view(NB, Sq, H, hstride)[..., :hp]).all()), "attention output: pad columns of the stored head"
    lse_ref = torch.logsumexp(s.detach(), -1) * 1.4426950408889634
    close(lse, lse_ref, 1e-3, 2e-2, "attention lse2")
    dq = poisoned((NB, Sq, D), BF, dev)
    out_dt = BF if (mask_block or bf16_out) else torch.float32
    dk = poisoned((NB, Sk, D), out_dt, dev); dv = poisoned((NB, Sk, D), out_dt, dev)
    ops.attn_gen_bwd(qd, kd, vd, o, dod, lse, dq, dk, dv, H, hp, hstride, scale, kv_len=kl, mask_block=mask_block)
    for got, r, nm in ((dq, qr.grad, "dq"), (dk, kr.grad, "dk"), (dv, vr.grad, "dv")):
        close(un(got), r, 3e-2, 2e-2 * _zero_ref_scale(r, vr.grad), "attention " + nm)
    untouched(dq.view(NB, Sq, H, hstride), stored(dq), "attention dq: columns past head_dim")
    if out_dt == BF:
        untouched(dk.view(NB, Sk, H, hstride), stored(dk), "attention dk: columns past head_dim")
        untouched(dv.view(NB, Sk, H, hstride), stored(dv), "attention dv: columns past head_dim")
        if kv_len is not None:
            for b, n in enumerate(kv_len):
                for t, nm in ((dk, "dk"), (dv, "dv")):
                    pad = t.view(NB, Sk, H, hstride)[b, n:, :, :hp]
                    assert bool((pad == 0).all()), f"attention {nm}: rows of sample {b} at and past kv_len = {n} must be exactly 0"


@pytest.mark.parametrize("NB,H,Sq,Sk", [(3, 2, 256, 256), (2, 3, 100, 77), (1, 16, 64, 64)])
def test_attn_gen_hd72(dev, NB, H, Sq, Sk):
    """STDiT spatial self-attention (blocks.py:139-225): 16 heads x 72, stored 80 wide"""
    _gen_case(dev, NB, H, Sq, Sk, 72, 80)


@pytest.mark.parametrize("NB,H,Sq,Sk,hd", [(3, 2, 256, 256, 72), (2, 3, 100, 77, 72), (2, 2, 333, 290, 72), (1, 2, 300, 300, 128)])
def test_attn_gen_bf16_dk_dv_written_whole(dev, NB, H, Sq, Sk, hd):
    """dK / dV straight to bf16 from the key-stationary pass (no accumulators to zero, no atomics): the form STDiT's spatial attention uses"""
    _gen_case(dev, NB, H, Sq, Sk, hd, 80 if hd == 72 else 128, bf16_out=True)


def test_attn_gen_many_queries_few_keys_split(dev):
    """STDiT's text cross-attention at its real aspect (4096 queries, <= 120 keys per sample): the query range is split over workgroups and
    dK / dV are summed with fp32 atomics"""
    _gen_case(dev, 2, 2, 4096, 120, 72, 80, kv_len=[37, 120])


def test_attn_gen_hd72_varlen_text(dev):
    """STDiT MultiHeadCrossAttention (blocks.py:472-505): every sample's queries against ITS first y_len text tokens"""
    _gen_case(dev, 3, 2, 300, 120, 72, 80, kv_len=[20, 120, 1])


@pytest.mark.parametrize("R,T", [(256, 16), (80, 16), (72, 8)])
def test_attn_gen_hd72_packed_temporal(dev, R, T):
    """STDiT temporal attention: R / T consecutive 16-frame sequences in one row space"""
    _gen_case(dev, 1, 4, R, R, 72, 80, mask_block=T)


@pytest.mark.parametrize("NB,H,Sq,Sk", [(1, 2, 300, 300), (2, 1, 130, 47)])
def test_attn_gen_hd128(dev, NB, H, Sq, Sk):
    """HunyuanVideo's head size (hyvideo_t2v/modules/attenion.py:60-156), short sequences"""
    _gen_case(dev, NB, H, Sq, Sk, 128, 128)


def test_attn_gen_hd128_packed(dev):
    """head_dim 128 with mask_block: 160 rows = ten 16-row sequences, a 128-row item plus a 32-row tail"""
    _gen_case(dev, 1, 2, 160, 160, 128, 128, mask_block=16)


def test_attn_gen_hd128_varlen(dev):
    """head_dim 128 with kv_len (fp32 dk / dv accumulators): all 47 keys, and a single key"""
    _gen_case(dev, 2, 1, 130, 47, 128, 128, kv_len=[47, 1])


@pytest.mark.parametrize("hd", [72, 128])
def test_attn_gen_bf16_dk_dv_varlen_padded_keys_get_zeros(dev, hd):
    """bf16 dK / dV written whole TOGETHER with kv_len: the poisoned rows at and past a sample's valid length come back exactly 0"""
    _gen_case(dev, 3, 2, 100, 77, hd, 80 if hd == 72 else 128, kv_len=[20, 77, 1], bf16_out=True)


@pytest.mark.parametrize("bf16_out", [False, True], ids=["fp32_dkdv", "bf16_dkdv"])
@pytest.mark.parametrize("NB,H,Sq,Sk", [(1, 1, 1, 1), (2, 2, 1, 77), (2, 2, 100, 1)])
@pytest.mark.parametrize("hd", [72, 128])
def test_attn_gen_one_query_one_key(dev, hd, NB, H, Sq, Sk, bf16_out):
    """a single query, a single key, and both: one lane of one tile is live"""
    _gen_case(dev, NB, H, Sq, Sk, hd, 80 if hd == 72 else 128, bf16_out=bf16_out)


@pytest.mark.parametrize("hd,hstride", [(72, 88), (128, 136)])
def test_attn_gen_heads_stored_wider_than_head_dim(dev, hd, hstride):
    """heads hstride > head_dim apart: the 8 columns between two heads belong to nobody and keep their poison (the kernels store 16-byte
    vectors per lane; a stray one lands exactly there)"""
    _gen_case(dev, 2, 2, 100, 77, hd, hstride)
    _gen_case(dev, 2, 2, 100, 77, hd, hstride, bf16_out=True)
    _gen_case(dev, 1, 2, 96, 96, hd, hstride, mask_block=16)


# ------------------------------------------------------------------------------------------------ operand packing
@pytest.mark.parametrize("R,C,ld", [(320, 1024, 1024), (72, 40, 48), (640, 640, 640), (8, 8, 8), (1280, 200, 256)])
def test_transpose_matches_torch(dev, R, C, ld):
    """vt_transpose_bf16: W^T of a Linear for its input gradient (row-strided source, ragged 64 x 64 tiles), bit-exact"""
    from vt355 import ops
    g = torch.Generator().manual_seed(R + C)
    buf = rb(torch.randn(R, ld, generator=g)).to(dev, BF)
    w = buf[:, :C]
    out = ops.transpose(w)
    assert out.is_contiguous() and torch.equal(out, w.t().contiguous())


def test_transpose_plan_runs_many_transposes_in_one_launch(dev):
    """ops.TransposePlan / vt_transpose_multi_bf16: a model's per-step operand packing as ONE launch -- Linear weights of several shapes
    (ragged 64 x 64 tiles, a row-strided source, a one-tile job between large ones) and the taps of two convolutions' input-gradient weights;
    every destination bit-equal to the single-weight paths; a second run after the sources changed refreshes all of them; operands that miss
    the alignment are refused (the caller keeps its own path)"""
    from vt355 import ops
    g = torch.Generator().manual_seed(9)
    plan = ops.TransposePlan(dev)
    lin, conv = [], []
    for R, C, ld in [(320, 320, 320), (1280, 320, 320), (8, 8, 8), (2560, 640, 640), (72, 200, 208), (1000, 136, 512)]:
        buf = rb(torch.randn(R, ld, generator=g)).to(dev, BF)
        src = buf[:, :C]
        dst = torch.full((C, R), 7.0, dtype=BF, device=dev)      # sentinel, not poison: every element must be overwritten by the plan (compared bit for bit below)
        assert plan.add(src, dst)
        lin.append((buf, src, dst))
    for Cout, Cin, kernel in [(320, 64, (3, 3)), (64, 320, (3, 1, 1))]:
        w = rb(torch.randn(Cout, Cin, *kernel, generator=g)).to(dev, BF)
        taps = math.prod(kernel)
        ws = ops.pack_conv_weight_nd(w).view(Cout, taps, Cin).contiguous()
        dst = torch.full((Cin, taps * Cout), 7.0, dtype=BF, device=dev)      # sentinel, not poison: every element must be overwritten by the plan (compared bit for bit below)
        assert plan.add_conv_dx(ws, dst)
        conv.append((ws, dst))
    odd = rb(torch.randn(12, 16, generator=g)).to(dev, BF)
    assert not plan.add(odd, poisoned((16, 12), BF, dev))                  # 12 rows: not a multiple of 8
    for rnd in range(2):
        plan.run()
        for buf, src, dst in lin:
            assert torch.equal(dst, src.t().contiguous())
        for ws, dst in conv:
            assert torch.equal(dst, ops.conv_weight_dx_from_storage(ws))
        for buf, src, dst in lin:
            buf.mul_(-0.5)
        for ws, dst in conv:
            ws.mul_(2.0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("Cout,Cin,kernel", [(320, 64, (3, 3)), (64, 320, (3, 1, 1)), (640, 320, (3, 3)), (8, 16, (3, 3))])
def test_conv_input_gradient_weight_from_storage(dev, Cout, Cin, kernel):
    """the input-gradient weight of a convolution (taps flipped, channels swapped) from the tap-major parameter storage in one batched
    transpose == pack_conv_weight_dx of the logical [Cout, Cin, *k] weight (flip + permute + contiguous), bit-exact"""
    from vt355 import ops
    g = torch.Generator().manual_seed(Cout + Cin)
    w = rb(torch.randn(Cout, Cin, *kernel, generator=g)).to(dev, BF)
    taps = math.prod(kernel)
    storage = ops.pack_conv_weight_nd(w).view(Cout, taps, Cin)            # what UNetModel keeps in its flat buffer
    got = ops.conv_weight_dx_from_storage(storage)
    assert torch.equal(got, ops.pack_conv_weight_dx(w))


# ------------------------------------------------------------------------------------------------ fp8 GEMM
@pytest.mark.parametrize("M,N,K", [(300, 256, 384), (4096, 3072, 3072), (77, 12, 128)])
def test_gemm_fp8_matches_dequantized_reference(dev, M, N, K):
    """real fp8 MFMA vs the reference's emulation (hunyuan fp8_optimization.py:55-80: E4M3 weight x per-tensor scale, de-quantised, F.linear),
    with the activation quantised the same way: bit-level agreement of the quantisers with torch's float8_e4m3fn cast, product within
    fp32-accumulation noise"""
    from vt355 import ops
    g = torch.Generator().manual_seed(M + N)
    a = rb(torch.randn(M, K, generator=g)); w = rb(torch.randn(N, K, generator=g) * 0.05); b = rb(torch.randn(N, generator=g))
    aq, sa = ops.quantize_fp8(a.to(dev, BF)); wq, sw = ops.quantize_fp8(w.to(dev, BF))
    sa_ref, sw_ref = a.abs().max() / 448.0, w.abs().max() / 448.0
    assert abs(sa.item() - sa_ref.item()) < 1e-6 * sa_ref.item() and abs(sw.item() - sw_ref.item()) < 1e-6 * sw_ref.item()
    aq_ref = (a / sa_ref).to(torch.float8_e4m3fn); wq_ref = (w / sw_ref).to(torch.float8_e4m3fn)
    assert (aq.cpu().view(torch.uint8) != aq_ref.view(torch.uint8)).float().mean().item() < 1e-3       # rounding ties aside
    ref = (aq.cpu().float() * sa.item()) @ (wq.cpu().float() * sw.item()).T + b
    out = poisoned((M, N), BF, dev)
    ops.gemm_fp8(aq, wq, out, sa, sw, b.to(dev, BF))
    close(out, ref, 1e-2, 1e-2 * ref.abs().max().item(), "fp8 GEMM")
    # and against the unquantised product: the quantisation error of E4M3 (3 mantissa bits) on both operands
    full = a @ w.T + b
    rel = ((out.float().cpu() - full).norm() / full.norm()).item()
    assert rel < 0.06, rel
