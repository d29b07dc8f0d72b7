"""lora_dropout for the CogVideoX DiT on the GPU: the six _drop rank-side kernels (csrc/lora.hip, csrc/lora_wide.hip) through vt355.ops,
and the training step through the module interface, against the CPU restatement of tests/lora_dropout_ref.py.

Exact kernel tests follow tests/test_side_kernels_gpu.py: small-integer inputs and p = 0.5, so 1 / (1 - p) = 2 and every product, partial
sum and result is an integer (or a multiple of alpha = 1/4) that fp32 holds exactly whatever the summation order; bf16 results stay within
|result| <= 256 (asserted on the reference).  Results are compared with torch.equal, outputs come from parity.poisoned, padding the kernel
must not read is NaN, what it must not write keeps a sentinel.  Every kernel test uses site0 = 116 (layer 29): the upper word of the
Philox counter is non-zero.  The expected masks are oracle/philox.py's dropout_keep_mask(M, K, p, seed, site << 36) on the LOGICAL width
K of the adapter input: a kernel that derived the element index from the row stride, the tile or the K block fails."""
import functools
import math

import numpy as np
import pytest
import torch

import lora_dropout_ref as R
from parity import all_written, close, poisoned, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")
SENT = 768.0
SEED, SITE0 = R.SEED, R.SITE0


def rb(x):
    return x.to(BF).float()


def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def sparse_ints(g, lo, hi, keep_one_in, *shape):
    """integers in [lo, hi], all but about one in keep_one_in set to zero (keeps |sum| small)"""
    return ints(g, lo, hi, *shape) * (torch.randint(0, keep_one_in, shape, generator=g) == 0).double()


def mask(M, K, p, site):
    return R.keep_mask(M, K, p, SEED, site)


def padded(t, ld, dev):
    """t [M, K] as a bf16 view of a [M, ld] device buffer whose padding columns are NaN"""
    buf = torch.full((t.shape[0], ld), NAN, dtype=BF, device=dev)
    buf[:, :t.shape[1]] = t.to(dev, BF)
    return buf[:, :t.shape[1]]


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


def layout(n, r):
    rp = (r + 15) // 16 * 16
    return rp, (n * rp + 63) // 64 * 64


# ================================================================== narrow layout (csrc/lora.hip)
ND_M, ND_K, ND_LDX = 100, 128, 192


@functools.lru_cache(maxsize=None)
def _down_data(R_rows):
    g = torch.Generator().manual_seed(40 + R_rows)
    return ints(g, -1, 1, ND_M, ND_K), ints(g, -1, 1, R_rows, ND_K)


def _down_ref(x, A, n, r, p, K):
    """[M, n r]: adapter j = 1/(1-p) (keep_j * x) A_j^T"""
    return torch.cat([(mask(x.shape[0], K, p, SITE0 + j) * x) @ A[j * r:(j + 1) * r].T / (1 - p) for j in range(n)], 1)


@pytest.mark.parametrize("r,n,calls", [(4, 3, 1), (7, 3, 3), (16, 1, 1)], ids=["r4x3_one_call", "r7x3_three_calls", "r16x1"])
def test_lora_down_drop_exact(dev, r, n, calls):
    """M = 100: two 64-row blocks, the second with 36 rows = two full 16-row tiles and one of 4; K = 128 = two K blocks; ldx = 192 with
    NaN padding.  x, A in {-1, 0, 1}: |T| <= 2 * 128 = 256.  r = 4: the three adapters share one call and one MFMA's rank columns under
    three masks.  r = 7: three calls as the engine issues them above 3 r = 16 (call j writes 16 columns from 7 j, zeros past its 7; the
    last zeroes the rest) on a poisoned extension.  r = 16: one adapter fills the MFMA."""
    from vt355 import ops
    x, A = _down_data(n * r)
    X = padded(x, ND_LDX, dev)
    T = poisoned((ND_M, 64), BF, dev)
    Ad = A.to(dev, BF)
    if calls == 1:
        ops.lora_down_drop(X, Ad, n * r, n, T, ND_K, 0.5, SEED, SITE0)
    else:
        for j in range(3):
            ops.lora_down_drop(X, Ad[j * r:(j + 1) * r], r, 1, T[:, j * r:], ND_K, 0.5, SEED, SITE0 + j,
                               zero_cols=(64 - 2 * r - 16) if j == 2 else 0)
    ref = _down_ref(x, A, n, r, 0.5, ND_K)
    assert ref.abs().max().item() <= 256
    all_written(T, "lora_down_drop")
    got = T.float().cpu().double()
    assert torch.equal(got[:, :n * r], ref), f"{(got[:, :n * r] != ref).sum().item()} of {ref.numel()} differ"
    assert (got[:, n * r:] == 0).all(), "the rest of the extension is not exactly 0"
    assert not torch.equal(ref, 2 * torch.cat([x @ A[j * r:(j + 1) * r].T for j in range(n)], 1)) and ref.abs().sum().item() > 0


def test_lora_down_drop_randn(dev):
    """randn x, 0.1 randn A at p = 0.1, r = 4 x 3 in one call, against fp64 on the bf16-rounded operands at test_lora_kernels' bar for
    lora_down (rtol 1e-2 / atol 1e-2 at K = 128)"""
    from vt355 import ops
    g = torch.Generator().manual_seed(61)
    x = rb(torch.randn(ND_M, ND_K, generator=g)).double(); A = rb(torch.randn(12, ND_K, generator=g) * 0.1).double()
    T = poisoned((ND_M, 64), BF, dev)
    ops.lora_down_drop(padded(x, ND_LDX, dev), A.to(dev, BF), 12, 3, T, ND_K, 0.1, SEED, SITE0)
    close(T[:, :12], _down_ref(x, A, 3, 4, 0.1, ND_K), 1e-2, 1e-2, "lora_down_drop randn")
    assert (T[:, 12:] == 0).all()


SK_M, SK_P, SK_LDB = 7100, 644, 712          # tests/test_side_kernels_gpu.py's rows37 geometry


@functools.lru_cache(maxsize=None)
def _skinny_data():
    g = torch.Generator().manual_seed(SK_M)
    return ints(g, -2, 2, SK_M, SK_P), ints(g, -2, 2, SK_M, 16)


@functools.lru_cache(maxsize=None)
def _skinny_masked(p):
    """the masked Big of the three sites, fp64 [3][M, P]"""
    big, _ = _skinny_data()
    return [mask(SK_M, SK_P, p, SITE0 + j) * big for j in range(3)]


def _skinny_ref(Rr, n, p, small):
    r = Rr // n
    mb = _skinny_masked(p)
    return torch.cat([mb[j].T @ small[:, j * r:(j + 1) * r] for j in range(n)], 1) / (1 - p)        # [P, R]


def _skinny_params():
    for Rr, n in ((4, 1), (12, 3), (16, 1)):
        for orient in ("out_PxR", "out_RxP"):
            for ws in (False, True):
                yield pytest.param(Rr, n, orient, ws, id=f"R{Rr}x{n}-{orient}-{'ws' if ws else 'atomics'}")
    for Rr in (3, 6, 9, 15):         # the other rank-column groupings of three adapters (r = 1, 2, 3, 5)
        yield pytest.param(Rr, 3, "out_RxP", False, id=f"R{Rr}x3-out_RxP-atomics")


@pytest.mark.parametrize("Rr,n,orient,use_ws", list(_skinny_params()))
def test_skinny_tn_drop_exact(dev, Rr, n, orient, use_ws):
    """out += 0.25 / (1 - 0.5) * sum_m keep_{i / r}(m, p) Big[m, p] Small[m, i] on integers in {-2..2}: multiples of 1/2 below 2^22, exact.
    M = 7100, P = 644, ldb = 712: 37 rows per slice = two 16-row unrolled groups and a 5-row tail, a second 512-column block with 132
    columns, NaN in the 68 padding columns of the row stride (the element index is m * 644 + p, not m * 712 + p).  R = 12 is the engine's
    one call for the three r = 4 adapters of the fused projection: rank columns 0-3, 4-7, 8-11 see three different masks of Big."""
    from vt355 import ops
    big, small = _skinny_data()
    bbuf = padded(big, SK_LDB, dev)
    sbuf = torch.full((SK_M, 8 + 16 + 8), NAN, dtype=BF, device=dev)
    sbuf[:, 8:8 + Rr] = small[:, :Rr].to(dev, BF)
    g = torch.Generator().manual_seed(Rr)
    out0 = ints(g, 1, 5, SK_P, Rr)
    expect = out0 + 0.25 * _skinny_ref(Rr, n, 0.5, small)
    assert torch.equal(expect.float().double(), expect)
    if orient == "out_PxR":
        buf = torch.full((SK_P, Rr + 3), SENT, device=dev); buf[:, :Rr] = out0.to(dev).float()
        out, osp, osr = buf[:, :Rr], Rr + 3, 1
    else:
        buf = torch.full((Rr, SK_P + 5), SENT, device=dev); buf[:, :SK_P] = out0.T.to(dev).float()
        out, osp, osr = buf[:, :SK_P], 1, SK_P + 5
    ops.skinny_tn_drop(bbuf, sbuf[:, 8:], Rr, n, out, osp, osr, 0.25, SK_P, 0.5, SEED, SITE0, use_workspace=use_ws)
    buf = buf.cpu().double()
    got, pad = (buf[:, :Rr], buf[:, Rr:]) if orient == "out_PxR" else (buf[:, :SK_P].T, buf[:, SK_P:])
    assert torch.equal(got, expect), f"{(got != expect).sum().item()} of {got.numel()} elements differ"
    assert (pad == SENT).all(), "wrote between the output strides"


def test_skinny_tn_drop_randn(dev):
    """randn operands, R = 12 (three adapters), p = 0.1, out [R, P], against fp64; bar as test_skinny_tn_randn: rtol 1e-3 and
    atol 1e-2 * sqrt(7100 / 333) scaled from test_lora_kernels' M = 333"""
    from vt355 import ops
    g = torch.Generator().manual_seed(72)
    big = rb(torch.randn(SK_M, SK_P, generator=g)).double(); small = rb(torch.randn(SK_M, 16, generator=g)).double()
    ref = torch.cat([(mask(SK_M, SK_P, 0.1, SITE0 + j) * big).T @ small[:, 4 * j:4 * j + 4] for j in range(3)], 1) / 0.9
    out = torch.zeros(12, SK_P, device=dev)
    ops.skinny_tn_drop(big.to(dev, BF), small.to(dev, BF), 12, 3, out, 1, SK_P, 1.0, SK_P, 0.1, SEED, SITE0)
    close(out, ref.T, 1e-3, 1e-2 * math.sqrt(7100 / 333), "skinny_tn_drop randn")


UA_M, UA_K = 100, 136


def _up_ref(dx, dt, A, n, r, p, K, col=lambda j, r: j * r):
    out = dx.clone()
    for j in range(n):
        out += mask(dx.shape[0], K, p, SITE0 + j) * (dt[:, col(j, r):col(j, r) + r] @ A[j * r:(j + 1) * r]) / (1 - p)
    return out


@pytest.mark.parametrize("Rr,n", [(4, 1), (12, 3), (16, 1)])
def test_lora_up_add_drop_exact(dev, Rr, n):
    """dX += 2 sum_j keep_j * (dT_j A_j) in place: dX in [-3, 3], dT in {-1, 0, 1}, A in {-2..2}: |result| <= 3 + 2 * 16 * 2 = 67.
    M = 100, K = 136 = 17 chunks of 8 (1700 chunks: 7 blocks, the last partial; the element index is m * 136 + k, ldx = 200).  dT is the
    extension of the same buffer, columns >= R NaN; the extension and a guard row above and below keep their bits."""
    from vt355 import ops
    g = torch.Generator().manual_seed(80 + Rr)
    dx, dt, A = ints(g, -3, 3, UA_M, UA_K), ints(g, -1, 1, UA_M, Rr), ints(g, -2, 2, Rr, UA_K)
    buf = torch.full((UA_M + 2, UA_K + 64), NAN, dtype=BF, device=dev)
    buf[0] = SENT; buf[-1] = SENT
    body = buf[1:UA_M + 1]
    body[:, :UA_K] = dx.to(dev, BF); body[:, UA_K:UA_K + Rr] = dt.to(dev, BF)
    ext_before = bits(body[:, UA_K:])
    ops.lora_up_add_drop(body, body[:, UA_K:], A.to(dev, BF), Rr, n, UA_K, 0.5, SEED, SITE0)
    ref = _up_ref(dx, dt, A, n, Rr // n, 0.5, UA_K)
    assert ref.abs().max().item() <= 256
    got = body[:, :UA_K].float().cpu().double()
    assert torch.equal(got, ref), f"{(got != ref).sum().item()} elements differ"
    assert not torch.equal(ref, dx + 2 * dt @ A)
    assert torch.equal(bits(body[:, UA_K:]), ext_before), "the extension columns changed"
    assert (buf[0] == SENT).all() and (buf[-1] == SENT).all(), "wrote outside the M rows"


def test_lora_up_add_drop_randn(dev):
    """randn at p = 0.1, three adapters of rank 4, at test_lora_kernels' bar for lora_up_add (rtol 1e-2 / atol 2e-2)"""
    from vt355 import ops
    g = torch.Generator().manual_seed(83)
    dx = rb(torch.randn(UA_M, UA_K, generator=g)).double(); A = rb(torch.randn(12, UA_K, generator=g) * 0.1).double()
    dt = rb(torch.randn(UA_M, 16, generator=g)).double()
    DX = dx.to(dev, BF).clone()
    ops.lora_up_add_drop(DX, dt.to(dev, BF), A.to(dev, BF), 12, 3, UA_K, 0.1, SEED, SITE0)
    close(DX, _up_ref(dx, dt, A, 3, 4, 0.1, UA_K), 1e-2, 2e-2, "lora_up_add_drop randn")


# ================================================================== wide layout (csrc/lora_wide.hip)
W_M, W_K, W_P = 200, 192, 136
WIDE = [(17, 32), (40, 48), (128, 128)]


@pytest.mark.parametrize("r,rp", WIDE)
def test_lora_down_wide_drop_exact(dev, r, rp):
    """M = 200 = three 64-row blocks and 8 rows (a partial 16-row tile), K = 192 = three K blocks (the sibling needs K % 64 == 0), ldx =
    200 with NaN padding.  Three adapters in one call for rp = 32 (tile t of adapter 16 t / 32: two tiles each) and rp = 48 (three tiles
    each, so a wave's tiles w, w + 4, w + 8 belong to three different adapters); rank 128 takes one adapter per call (three masked X
    blocks and 384 rows of A exceed the 64 KB of LDS), as the engine then calls it.  x in {-1, 0, 1}, A in {-1, 0, 1} with one in two
    entries zero keeps |T| <= 256 (asserted).  Padding columns and the rest of the extension must be exactly 0 on a poisoned buffer."""
    from vt355 import ops
    n = 3 if ops.lora_down_wide_drop_fits(3, rp) else 1
    assert n == (1 if rp == 128 else 3)
    _, ext = layout(n, r)
    g = torch.Generator().manual_seed(90 + r)
    x, A = ints(g, -1, 1, W_M, W_K), sparse_ints(g, -1, 1, 2, n * r, W_K)
    T = poisoned((W_M, ext), BF, dev)
    ops.lora_down_wide_drop(padded(x, W_K + 8, dev), A.to(dev, BF), n, r, rp, ext, T, W_K, 0.5, SEED, SITE0)
    all_written(T, "lora_down_wide_drop")
    ref = torch.zeros(W_M, ext, dtype=torch.float64)
    for j in range(n):
        ref[:, j * rp:j * rp + r] = 2 * (mask(W_M, W_K, 0.5, SITE0 + j) * x) @ A[j * r:(j + 1) * r].T
    assert ref.abs().max().item() <= 256 and ref.abs().sum().item() > 0
    got = T.float().cpu().double()
    assert torch.equal(got, ref), f"{(got != ref).sum().item()} of {ref.numel()} differ"


@pytest.mark.parametrize("Rr", [17, 40, 128])
@pytest.mark.parametrize("orient", ["osr1", "osp1"])
def test_lora_tn_wide_drop_exact(dev, Rr, orient):
    """out += 0.25 * 2 * sum_m keep(m, p) Big[m, p] Small[m, i]: M = 200 (3 row tiles of 64 and one of 8), P = 136 = one 128-column block
    and 8 columns of a second, ldb = 144 with NaN padding (element index m * 136 + p); both output orientations; integers in {-2..2}"""
    from vt355 import ops
    g = torch.Generator().manual_seed(7 * Rr)
    big, small = ints(g, -2, 2, W_M, W_P), ints(g, -2, 2, W_M, Rr)
    sbuf = torch.full((W_M, 16 + Rr + 5), NAN, dtype=BF, device=dev); sbuf[:, 16:16 + Rr] = small.to(dev, BF)
    out0 = ints(g, 1, 5, W_P, Rr)
    expect = out0 + 0.5 * (mask(W_M, W_P, 0.5, SITE0) * big).T @ small
    if orient == "osr1":
        buf = torch.full((W_P, Rr + 3), SENT, device=dev); buf[:, :Rr] = out0.to(dev).float()
        ops.lora_tn_wide_drop(padded(big, 144, dev), sbuf[:, 16:], Rr, buf[:, :Rr], Rr + 3, 1, 0.25, W_P, 0.5, SEED, SITE0)
        got, pad = buf[:, :Rr].cpu().double(), buf[:, Rr:]
    else:
        buf = torch.full((Rr, W_P + 5), SENT, device=dev); buf[:, :W_P] = out0.T.to(dev).float()
        ops.lora_tn_wide_drop(padded(big, 144, dev), sbuf[:, 16:], Rr, buf[:, :W_P], 1, W_P + 5, 0.25, W_P, 0.5, SEED, SITE0)
        got, pad = buf[:, :W_P].T.cpu().double(), buf[:, W_P:]
    assert torch.equal(got, expect), f"{(got != expect).sum().item()} of {got.numel()} elements differ"
    assert (pad == SENT).all()


@pytest.mark.parametrize("r,rp", WIDE)
def test_lora_up_add_wide_drop_exact(dev, r, rp):
    """dX += 2 sum_j keep_j * (dT_j A_j), three adapters in one pass: M = 200 (a 128-row block and 72 rows: wave 2 of the second block has
    8 rows, wave 3 none), K = 192.  rp = 48: adapters end at columns 48 and 96 + 48 = 144, in the middle of the 32-deep steps 1 and 4, so
    the dT fragments of the other adapter's lanes must be zeroed.  dX in [-3, 3]; dT and A in {-1, 0, 1}, one in two (dT) / four (A) entries
    non-zero keeps |result| <= 256 (asserted)."""
    from vt355 import ops
    n = 3
    _, ext = layout(n, r)
    g = torch.Generator().manual_seed(95 + r)
    dx, A = ints(g, -3, 3, W_M, W_K), sparse_ints(g, -1, 1, 4, n * r, W_K)
    dt = torch.zeros(W_M, ext, dtype=torch.float64)
    for j in range(n):
        dt[:, j * rp:j * rp + r] = sparse_ints(g, -1, 1, 2, W_M, r)
    buf = torch.full((W_M + 2, W_K + ext), SENT, dtype=BF, device=dev)
    body = buf[1:W_M + 1]
    body[:, :W_K] = dx.to(dev, BF); body[:, W_K:] = dt.to(dev, BF)
    ext_before = bits(body[:, W_K:])
    ops.lora_up_add_wide_drop(body, body[:, W_K:], A.to(dev, BF), n, r, rp, W_K, 0.5, SEED, SITE0)
    ref = _up_ref(dx, dt, A, n, r, 0.5, W_K, col=lambda j, r_: j * rp)
    assert ref.abs().max().item() <= 256
    got = body[:, :W_K].float().cpu().double()
    assert torch.equal(got, ref), f"{(got != ref).sum().item()} elements differ"
    assert torch.equal(bits(body[:, W_K:]), ext_before)
    assert (buf[0] == SENT).all() and (buf[-1] == SENT).all()


def test_wide_drop_randn(dev):
    """one randn case per wide kernel at p = 0.1 against fp64, at the bars tests/test_lora_wide_gpu.py took from test_lora_kernels:
    down 1e-2 / 1e-2, rank gradients 1e-3 / 1e-2, up-add 1e-2 / 2e-2"""
    from vt355 import ops
    g = torch.Generator().manual_seed(99)
    n, r, rp = 3, 40, 48
    _, ext = layout(n, r)
    x = rb(torch.randn(W_M, W_K, generator=g)).double(); A = rb(torch.randn(n * r, W_K, generator=g) * 0.1).double()
    T = poisoned((W_M, ext), BF, dev)
    ops.lora_down_wide_drop(x.to(dev, BF), A.to(dev, BF), n, r, rp, ext, T, W_K, 0.1, SEED, SITE0)
    for j in range(n):
        close(T[:, j * rp:j * rp + r], (mask(W_M, W_K, 0.1, SITE0 + j) * x) @ A[j * r:(j + 1) * r].T / 0.9, 1e-2, 1e-2, f"down_wide_drop {j}")
    big = rb(torch.randn(W_M, W_P, generator=g)).double(); small = rb(torch.randn(W_M, r, generator=g)).double()
    out = torch.zeros(W_P, r, device=dev)
    ops.lora_tn_wide_drop(big.to(dev, BF), small.to(dev, BF), r, out, r, 1, 0.25, W_P, 0.1, SEED, SITE0)
    close(out, 0.25 * (mask(W_M, W_P, 0.1, SITE0) * big).T @ small / 0.9, 1e-3, 1e-2, "tn_wide_drop")
    dx = rb(torch.randn(W_M, W_K, generator=g)).double()
    dt = torch.zeros(W_M, ext, dtype=torch.float64)
    for j in range(n):
        dt[:, j * rp:j * rp + r] = rb(torch.randn(W_M, r, generator=g)).double()
    DX = torch.cat([dx, dt], 1).to(dev, BF)
    ops.lora_up_add_wide_drop(DX, DX[:, W_K:], A.to(dev, BF), n, r, rp, W_K, 0.1, SEED, SITE0)
    close(DX[:, :W_K], _up_ref(dx, dt, A, n, r, 0.1, W_K, col=lambda j, r_: j * rp), 1e-2, 2e-2, "up_add_wide_drop")


# ================================================================== the mask, from a second source on the device
@pytest.mark.parametrize("p", [0.5, 0.1])
def test_kernel_masks_equal_vt_dropout_bf16(dev, p):
    """x = 1 and A = the identity on r columns make T[m, i] = keep(m, i) / (1 - p): the mask the down kernels imply must be the one
    vt_dropout_bf16 exports at the same (seed, offset = site << 36), for the narrow (r = 16, K = 128) and the wide (r = 128, K = 192)
    kernel, and both must be oracle/philox.py's."""
    from vt355 import ops
    for wide, K, r in ((False, ND_K, 16), (True, W_K, 128)):
        M = W_M
        ones = torch.ones(M, K, dtype=BF, device=dev)
        y = poisoned((M, K), BF, dev); mk = poisoned((M, K), torch.uint8, dev)
        ops.dropout(ones, y, p, SEED, offset=(SITE0 + 1) << 36, mask_out=mk)
        A = torch.zeros(r, K, dtype=BF, device=dev); A[torch.arange(r), torch.arange(r)] = 1
        if wide:
            T = poisoned((M, 128), BF, dev)
            ops.lora_down_wide_drop(ones, A, 1, r, 128, 128, T, K, p, SEED, SITE0 + 1)
        else:
            T = poisoned((M, 64), BF, dev)
            ops.lora_down_drop(ones, A, r, 1, T, K, p, SEED, SITE0 + 1)
        implied = (T[:, :r] != 0).to(torch.uint8)
        assert torch.equal(implied, mk[:, :r]), f"wide={wide}: {(implied != mk[:, :r]).sum().item()} mask bits differ from vt_dropout_bf16's"
        assert torch.equal(mk.cpu(), torch.from_numpy(np.ascontiguousarray(R._mask_np(M, K, float(p), SEED, SITE0 + 1))))
        assert torch.equal(T[:, :r], y[:, :r]), "kept elements are not 1 / (1 - p) rounded once"


def test_drop_entry_points_refuse_bad_arguments(dev):
    from vt355 import ops
    from vt355._lib import VtError
    x = torch.zeros(64, 128 + 64, dtype=BF, device=dev); a = torch.zeros(48, 128, dtype=BF, device=dev)
    out = torch.zeros(12, 128, device=dev)
    for p in (1.0, -0.1, float("nan")):
        with pytest.raises(VtError):
            ops.lora_down_drop(x, a, 12, 3, x[:, 128:], 128, p, 1, 0)
        with pytest.raises(VtError):
            ops.skinny_tn_drop(x, x[:, 128:], 12, 3, out, 1, 128, 1.0, 128, p, 1, 0)
        with pytest.raises(VtError):
            ops.lora_up_add_drop(x, x[:, 128:], a, 12, 3, 128, p, 1, 0)
        with pytest.raises(VtError):
            ops.lora_down_wide_drop(x, a, 1, 17, 32, 64, x[:, 128:], 128, p, 1, 0)
        with pytest.raises(VtError):
            ops.lora_tn_wide_drop(x, x[:, 128:], 12, out, 1, 128, 1.0, 128, p, 1, 0)
        with pytest.raises(VtError):
            ops.lora_up_add_wide_drop(x, x[:, 128:], a, 1, 17, 32, 128, p, 1, 0)
    with pytest.raises(VtError):
        ops.lora_down_drop(x, a, 12, 5, x[:, 128:], 128, 0.1, 1, 0)             # 12 rank columns do not split into 5 adapters
    with pytest.raises(VtError):
        ops.lora_down_wide_drop(x, a, 3, 128, 128, 384, x[:, 128:], 128, 0.1, 1, 0)   # three masked X blocks at rank 128 exceed the LDS
    with pytest.raises(ValueError):
        ops.lora_down_drop(x.cpu(), a, 12, 3, x[:, 128:], 128, 0.1, 1, 0)       # host tensor


# ================================================================== the model
def _device_step(dev, r, p, rope=False, b_random=True, recompute="never", seed=SEED):
    """selfcheck.tiny_train_step_check's step with lora_dropout p and a pinned seed; returns what the comparisons need"""
    from selfcheck import build_tiny
    from vt355.scheduler import CogVideoXDPMScheduler
    from vt355.workflow import _LossFn
    cfg, model, peft, st = build_tiny(dev, use_rotary_positional_embeddings=rope, lora_r=r, lora_b_random=b_random)
    st.p = p
    model.lora_dropout_seed = seed
    model.enable_gradient_checkpointing(recompute)
    x0, text, noise, t = R.tiny_inputs(cfg)
    sched = CogVideoXDPMScheduler()
    noisy = sched.add_noise(x0.to(dev), noise.to(dev), t.to(dev))
    tabs = R.rope_tables(cfg, rope)
    sa, sb, w = sched.coefficients(t.to(dev))

    def run():
        st.grad.zero_()
        out = peft(hidden_states=noisy, encoder_hidden_states=text.to(dev), timestep=t.to(dev), return_dict=False,
                   image_rotary_emb=None if tabs is None else (tabs[0].to(dev), tabs[1].to(dev)))[0]
        loss = _LossFn.apply(out, noisy, x0.to(dev), sa, sb, w)
        loss.backward()
        names = [f"transformer_blocks.{layer}.attn1.{R.TARGETS[j]}.lora_{kind}.default.weight" for (layer, kind, j) in st._index]
        grads = {n: st.view(st.grad, layer, kind, j).detach().cpu().double().clone() for n, (layer, kind, j) in zip(names, st._index)}
        return loss.item(), grads, out
    return dict(cfg=cfg, model=model, peft=peft, st=st, run=run, x0=x0, text=text, t=t, tabs=tabs, noisy=noisy.float().cpu().double())


@pytest.mark.parametrize("r,p,rope", [(4, 0.1, False), (4, 0.5, False), (8, 0.1, False), (8, 0.5, False), (20, 0.1, False),
                                      (20, 0.5, False), (40, 0.1, False), (40, 0.5, False), (128, 0.1, False), (4, 0.5, True), (40, 0.1, True)])
def test_train_step_matches_the_dropped_reference(dev, r, p, rope, monkeypatch):
    """loss and adapter gradients of the tiny training step (B = 2, random B, pinned seed) against the fp64 oracle with lora_dropout
    patched in, at tiny_train_step_check's bars: loss 2e-2 relative, gradients rel-L2 6e-2 and cosine > 0.995.  r = 4: one narrow call
    for q, k, v; r = 8: three; r = 20 (rp = 32), 40 (rp = 48): wide; r = 128: wide with one down-projection call per adapter; rope: the
    5B layout.  At p = 0.5 each of the three wrong references
    must fail the same bars."""
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False); monkeypatch.delenv("VT355_RECOMPUTE", raising=False)
    s = _device_step(dev, r, p, rope)
    loss, grads, _ = s["run"]()
    assert s["model"].last_lora_dropout_seed == SEED
    ref = lambda variant: R.reference_step(monkeypatch, s["cfg"], s["model"], s["st"], s["noisy"], s["x0"], s["text"], s["t"], p, SEED,
                                           variant, s["tabs"])
    loss_ref, gref = ref("right")
    rel, cos = R.overall(R.flat(grads, list(gref)), R.flat(gref))
    worst = max((rel_l2(grads[k], gref[k]), k) for k in gref)
    print(f"r={r} p={p} rope={rope}: loss {loss:.6f} ref {loss_ref:.6f}; grads rel-L2 {rel:.3e} cos {cos:.5f}; worst adapter {worst[0]:.3e} {worst[1]}")
    assert abs(loss - loss_ref) / abs(loss_ref) < 2e-2, (loss, loss_ref)
    assert rel < 6e-2 and cos > 0.995, (rel, cos)
    if p == 0.5:
        for variant in R.VARIANTS[1:]:
            lw, gw = ref(variant)
            relw, cosw = R.overall(R.flat(grads, list(gw)), R.flat(gw))
            print(f"   against {variant}: grads rel-L2 {relw:.3e} cos {cosw:.5f}, loss rel {abs(loss - lw) / abs(lw):.2e}")
            assert not (relw < 6e-2 and cosw > 0.995), (variant, relw, cosw)


@pytest.mark.parametrize("r", [4, 8, 40])
def test_recompute_uses_the_same_masks(dev, r, monkeypatch):
    """enable_gradient_checkpointing("always") runs every block's forward a second time in the backward pass: with the forward's seed on
    the saved state the loss is the same bit for bit and the gradients agree up to the order of the fp32 atomic adds (rel-L2 < 1e-3,
    test_block_recompute_gives_the_same_gradients' tolerance)."""
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False); monkeypatch.delenv("VT355_RECOMPUTE", raising=False)
    s = _device_step(dev, r, 0.1)
    l0, g0, _ = s["run"]()
    s["model"].enable_gradient_checkpointing("always")
    l1, g1, _ = s["run"]()
    assert l0 == l1
    rel = rel_l2(R.flat(g1), R.flat(g0))
    assert R.flat(g0).abs().max().item() > 0 and rel < 1e-3, rel


@pytest.mark.parametrize("r", [4, 40])
def test_eval_and_seeds(dev, r, monkeypatch):
    """model.eval() switches the masks off: the prediction with p = 0.1 is torch.equal to the one of the same weights with p = 0.  In
    training mode a pinned seed gives the same loss bits twice and a loss different from p = 0; unpinned forwards draw different seeds."""
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False); monkeypatch.delenv("VT355_RECOMPUTE", raising=False)
    s = _device_step(dev, r, 0.1)
    peft, model, st = s["peft"], s["model"], s["st"]
    l0, _, out_train = s["run"]()
    l1, _, _ = s["run"]()
    assert l0 == l1
    st.p = 0.0
    l_nodrop, _, out_nodrop = s["run"]()
    assert l_nodrop != l0 and not torch.equal(out_train, out_nodrop)
    peft.eval()
    assert not model.training
    st.p = 0.1
    _, _, out_eval = s["run"]()
    assert torch.equal(out_eval, out_nodrop)
    peft.train()
    model.lora_dropout_seed = None
    seeds = set()
    for _ in range(3):
        s["run"]()
        seeds.add(model.last_lora_dropout_seed)
    assert len(seeds) == 3 and all(0 <= x < 2 ** 62 for x in seeds)


def test_zero_b_init(dev, monkeypatch):
    """peft's init (B = 0): T never reaches the output, so dT = 0 and dA is exactly 0, while dB = dY^T T sees the dropped T and differs from
    the p = 0 run"""
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False); monkeypatch.delenv("VT355_RECOMPUTE", raising=False)
    s = _device_step(dev, 4, 0.1, b_random=False)
    _, g, _ = s["run"]()
    s["st"].p = 0.0
    _, g0, _ = s["run"]()
    for k in g:
        if "lora_A" in k:
            assert (g[k] == 0).all(), k
        else:
            assert g[k].abs().max().item() > 0 and not torch.equal(g[k], g0[k]), k
