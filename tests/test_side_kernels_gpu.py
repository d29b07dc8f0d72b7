"""Exact-result tests of the LoRA rank-side kernels (csrc/lora.hip, ranks 1..16) and of the one-row-per-sample backward
kernels (csrc/reduce.hip, csrc/elementwise.hip), all called through vt355.ops.

Wherever a kernel accumulates products in fp32 and stores fp32, the inputs are SMALL INTEGERS (exact in bf16) and alpha is a
power of two: every product and every partial sum is an integer (or a multiple of alpha) below 2^24, hence exact in fp32
whatever the summation order, the slicing or the atomics.  Such results are compared with torch.equal against an fp64 CPU
reference -- no tolerance: one dropped, duplicated or misplaced row, column or lane fails.  Kernels that store bf16 get inputs
that keep |result| <= 256, so the bf16 store is exact too.  Every input the kernel must not read is NaN, every element it
must not write holds a sentinel that is asserted afterwards.  One randn case per kernel at the project's existing bars
(tests/test_kernels_gpu.py) exercises non-integer rounding.

The docstrings name the code path a shape reaches and give the arithmetic against the constants of the kernels
(SK_SLICES = 192, SK_MAXROWS = 512, 512-column blocks, the 8192 / 1024 / 512-block grid caps ...): if those constants change,
the shapes here must be revisited.  The tests never read or set the VT_SK_SLICES / VT_RD_SLICES overrides."""
import functools
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cogvideox_oracle as O
from parity import close, poisoned

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")
SENT = 768.0          # sentinel of elements a kernel must not write (exact in bf16 and fp32)


def rb(x):      # bf16-round but keep fp32 (what the device kernel actually sees)
    return x.to(BF).float()


def ints(g, lo, hi, *shape):
    """uniform integers in [lo, hi] as fp64"""
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def bits(t):
    """the raw 16-bit patterns of a bf16 tensor (NaN-safe bitwise comparison)"""
    return t.contiguous().view(torch.int16).cpu()


def _lora_state(r, a_bf16=None, grad=None):
    """what engine._lora_down_qkv / _lora_qkv_input_grads read of a LoraState (narrow layout, one layer)"""
    return SimpleNamespace(r=r, wide=False, rp=r, ext_qkv=64, flat_bf16=a_bf16, grad=grad, a_qkv=lambda flat, i: flat)


# ================================================================== A. csrc/lora.hip
# ------------------------------------------------------------------ 1. skinny_tn
SK_CASES = {           # name: (M, P, ldb)
    "rows37": (7100, 644, 712),
    "two_launches": (98819, 128, 128),
    "empty_slices": (100, 512, 512),
}


@functools.lru_cache(maxsize=None)
def _skinny_data(case):
    """integer Big [M, P], Small [M, 16] in {-2..2} and the exact fp64 product Big^T Small [P, 16], computed once per case"""
    M, P, _ = SK_CASES[case]
    g = torch.Generator().manual_seed(M)
    big, small = ints(g, -2, 2, M, P), ints(g, -2, 2, M, 16)
    return big, small, big.T @ small


@functools.lru_cache(maxsize=None)
def _skinny_dev(case, dev):
    M, P, ldb = SK_CASES[case]
    big, small, _ = _skinny_data(case)
    bbuf = torch.full((M, ldb), NAN, dtype=BF, device=dev)          # padding columns of the row stride: NaN
    bbuf[:, :P] = big.to(dev, BF)
    return bbuf, small.to(dev, BF)


def _skinny_params():
    for case in SK_CASES:
        for R in ((4, 16) if case == "two_launches" else (1, 4, 5, 12, 16)):
            for orient in ("out_PxR", "out_RxP"):
                for ws in (False, True):
                    yield pytest.param(case, R, orient, ws, id=f"{case}-R{R}-{orient}-{'ws' if ws else 'atomics'}")


@pytest.mark.parametrize("case,R,orient,use_ws", list(_skinny_params()))
def test_skinny_tn_exact(dev, case, R, orient, use_ws):
    """out += 0.25 * Big^T Small on integers in {-2..2}: |sum| <= 4 M < 2^24 and alpha = 2^-2, so out is exact (torch.equal).

    rows37 (M = 7100, P = 644, ldb = 712): rows per slice = ceil(7100 / 192) = 37 = two 16-row unrolled groups + a 5-row tail
      (the 16-to-tail hand-over); 191 slices x 37 = 7067, the last slice has 33 rows = 16 + 16 + 1.  P = 644 is a second
      512-column block with 132 valid columns = 33 of its 128 threads.  The 68 padding columns of ldb are NaN.
    two_launches (M = 98 819, P = 128): 192 x 512 = 98 304 rows per launch, so the mbase loop runs twice: 512 rows per slice
      (32 unrolled groups, the whole LDS staging) and a 515-row remainder = 3 rows per slice, 171 x 3 + 2, 20 empty slices.
    empty_slices (M = 100, P = 512): 1 row per slice, slices 100..191 have no rows.
    R in {1, 4} runs skinny_tn_kernel<4> (with and without the workspace), R in {5, 12, 16} <16>.  out_PxR is osr == 1 with a
    row stride of R + 3 (engine_fullft._dw: gw.view(-1)[c:], osp = Q), out_RxP is the osp == 1 transposed-atomics branch with
    a row stride of P + 5; the elements between the strides keep their sentinel.  Small is a column-offset view of a wider
    buffer (dx1[:, d + j*r:] in the engine) whose columns >= R are NaN; out starts from non-zero integers (the contract is +=).
    With the workspace the same call is issued twice on the same start values and must give identical bits."""
    from vt355 import ops
    M, P, ldb = SK_CASES[case]
    _, _, prod = _skinny_data(case)
    bbuf, small16 = _skinny_dev(case, dev)
    sbuf = torch.full((M, 8 + 16 + 8), NAN, dtype=BF, device=dev)
    sbuf[:, 8:8 + R] = small16[:, :R]
    g = torch.Generator().manual_seed(R)
    out0 = ints(g, 1, 5, P, R)
    expect = (out0 + 0.25 * prod[:, :R]).float()                     # exact: multiples of 1/4 below 2^22
    assert torch.equal(expect.double(), out0 + 0.25 * prod[:, :R])

    def run():
        if orient == "out_PxR":
            buf = torch.full((P, R + 3), SENT, device=dev); buf[:, :R] = out0.to(dev).float()
            out, osp, osr = buf[:, :R], R + 3, 1
        else:
            buf = torch.full((R, P + 5), SENT, device=dev); buf[:, :P] = out0.T.to(dev).float()
            out, osp, osr = buf[:, :P], 1, P + 5
        ops.skinny_tn(bbuf[:, :P], sbuf[:, 8:], R, out, osp, osr, 0.25, P, use_workspace=use_ws)
        return buf.cpu()
    buf = run()
    got, pad = (buf[:, :R], buf[:, R:]) if orient == "out_PxR" else (buf[:, :P].T, buf[:, P:])
    assert torch.equal(got, expect), f"{(got != expect).sum().item()} of {got.numel()} elements differ"
    assert (pad == SENT).all(), "wrote between the output strides"
    if use_ws:
        assert torch.equal(run(), buf), "the two-stage reduction is not bitwise reproducible"


@pytest.mark.parametrize("use_ws", [False, True], ids=["atomics", "ws"])
def test_skinny_tn_randn(dev, use_ws):
    """randn operands at (M, P, R) = (7100, 644, 12), out [R, P], against fp64 on the same bf16-rounded inputs.  Bar: the existing
    one of test_lora_kernels, rtol 1e-3 / atol 1e-2 at M = 333; the result is a sum of M independent products, so its size and
    the fp32 accumulation error grow as sqrt(M): atol = 1e-2 * sqrt(7100 / 333) = 4.62e-2."""
    from vt355 import ops
    M, P, R = 7100, 644, 12
    g = torch.Generator().manual_seed(71)
    big = rb(torch.randn(M, P, generator=g)); small = rb(torch.randn(M, 16, generator=g))
    ref = small[:, :R].double().T @ big.double()
    sm = small.to(dev, BF); sm[:, R:] = NAN
    out = torch.zeros(R, P, device=dev)
    ops.skinny_tn(big.to(dev, BF), sm, R, out, 1, P, 1.0, P, use_workspace=use_ws)
    close(out, ref, 1e-3, 1e-2 * math.sqrt(7100 / 333), "skinny_tn randn")


# ------------------------------------------------------------------ 2. lora_down
LD_M, LD_K = 333, 1920


def _lora_down_run(dev, x, A, r):
    """the engine's own call pattern (engine._lora_down_qkv) on a [M, K + 64] buffer whose extension is all NaN"""
    from vt355 import engine
    X = torch.full((LD_M, LD_K + 64), NAN, dtype=BF, device=dev)
    X[:, :LD_K] = x.to(dev, BF)
    before = bits(X[:, :LD_K])
    engine._lora_down_qkv(X, _lora_state(r, a_bf16=A.to(dev, BF)), 0, LD_K)
    assert torch.equal(bits(X[:, :LD_K]), before), "the base columns [0, K) changed"
    assert (X[:, LD_K + 3 * r:] == 0).all(), "columns [K + 3r, K + 64) are not exactly 0"
    return X[:, LD_K:LD_K + 3 * r].float().cpu()


@pytest.mark.parametrize("r", [1, 4, 5, 6, 8, 11, 16])
def test_lora_down_exact(dev, r):
    """T = x A^T into the K-extension, M = 333 (6 blocks of 64 rows; the last has 13 rows: 320..332, so the row clamp and the
    m < M store guards run), K = 1920 = 30 K iterations of 64.
    r in {1, 4, 5}: one call with R = 3r and zero_cols = 48.  r in {6, 8, 11, 16}: the three q / k / v calls exactly as
    engine._lora_down_qkv issues them -- call j writes 16 columns from j*r (zeros past its r), call j+1 overwrites the zeros call
    j left in its columns, the last call zeroes the remaining EXT - 2r - 16.  The extension starts as NaN, so a column nobody
    wrote, or a zero that was not overwritten, shows.
    Exact: x in {-1, 0, 1}; row i of A has 64 entries of +-1, at k = 64 * ((c + i) % 30) + c for c = 0..63, i.e. every k mod 64
    lane position and every one of the 30 K blocks (the last included) in every row; |T| <= 64, exact in bf16."""
    g = torch.Generator().manual_seed(100 + r)
    x = ints(g, -1, 1, LD_M, LD_K)
    A = torch.zeros(3 * r, LD_K, dtype=torch.float64)
    c = torch.arange(64)
    for i in range(3 * r):
        A[i, 64 * ((c + i) % 30) + c] = ints(g, 0, 1, 64) * 2 - 1
    T = _lora_down_run(dev, x, A, r)
    assert torch.equal(T.double(), x @ A.T)


@pytest.mark.parametrize("r", [4, 8], ids=["one_call_r4", "three_calls_r8"])
def test_lora_down_randn(dev, r):
    """randn x, 0.1 * randn A as in test_lora_kernels, whose bar is rtol 1e-2 / atol 1e-2 at K = 128; T is a sum of K products,
    its size grows as sqrt(K): atol = 1e-2 * sqrt(1920 / 128) = 3.87e-2."""
    g = torch.Generator().manual_seed(200 + r)
    x = rb(torch.randn(LD_M, LD_K, generator=g)); A = rb(torch.randn(3 * r, LD_K, generator=g) * 0.1)
    T = _lora_down_run(dev, x, A, r)
    close(T, x.double() @ A.double().T, 1e-2, 1e-2 * math.sqrt(1920 / 128), "lora_down randn")


# ------------------------------------------------------------------ 3. lora_up_add
@functools.lru_cache(maxsize=None)
def _up_add_data(M, K):
    g = torch.Generator().manual_seed(M + K)
    return ints(g, -3, 3, M, K), ints(g, -1, 1, M, 16), ints(g, -2, 2, 16, K)


@pytest.mark.parametrize("R", [1, 12, 16])
@pytest.mark.parametrize("M,K", [(9001, 1920), (77, 64)])
def test_lora_up_add_exact(dev, M, K, R):
    """dX += dT A in place (bf16): dX in [-3, 3], dT in {-1, 0, 1}, A in {-2..2}, so |result| <= 3 + 16 * 2 = 35 is exact in bf16.
    M = 9001, K = 1920: 9001 * 240 = 2 160 240 8-element chunks against the grid cap of 8192 blocks x 256 = 2 097 152 threads:
    63 088 threads take a second trip of the grid-stride loop.  M = 77, K = 64: 616 chunks, 3 blocks, the last one partial.
    ldx = K + 64 and dT is the extension view of the same buffer, as in the engine; extension columns >= R are NaN (never read).
    The extension and a guard row above and below must keep their bits."""
    from vt355 import ops
    dx, dt, a = _up_add_data(M, K)
    buf = torch.full((M + 2, K + 64), NAN, dtype=BF, device=dev)
    buf[0] = SENT; buf[-1] = SENT
    body = buf[1:M + 1]
    body[:, :K] = dx.to(dev, BF); body[:, K:K + R] = dt[:, :R].to(dev, BF)
    ext_before = bits(body[:, K:])
    ops.lora_up_add(body, body[:, K:], a.to(dev, BF), R, K)
    expect = (dx + dt[:, :R] @ a[:R]).to(dev, BF)
    assert torch.equal(body[:, :K], expect), f"{(body[:, :K] != expect).sum().item()} elements differ"
    assert torch.equal(bits(body[:, K:]), ext_before), "the extension columns changed"
    assert (buf[0] == SENT).all() and (buf[-1] == SENT).all(), "wrote outside the M rows"


def test_lora_qkv_input_grads_sequence_exact(dev):
    """rank 8: the three per-adapter skinny_tn + lora_up_add calls of engine._lora_qkv_input_grads (adapter j reads the 8
    extension columns from j*8) must equal ONE fp64 dA_all = dT_all^T x1 and dx1 += dT_all A_all.  M = 333, d = 128; integers, so
    both are exact: |dA| <= 2 * 333 on top of non-zero start values, |dx1| <= 3 + 24 * 2 = 51.  Extension columns >= 24 are NaN."""
    from vt355 import engine
    M, d, r = 333, 128, 8
    g = torch.Generator().manual_seed(38)
    x1, dx, dt = ints(g, -2, 2, M, d), ints(g, -3, 3, M, d), ints(g, -1, 1, M, 3 * r)
    A, dA0 = ints(g, -2, 2, 3 * r, d), ints(g, 1, 5, 3 * r, d)
    X1 = torch.full((M, d + 64), NAN, dtype=BF, device=dev); X1[:, :d] = x1.to(dev, BF)
    DX = torch.full((M, d + 64), NAN, dtype=BF, device=dev); DX[:, :d] = dx.to(dev, BF); DX[:, d:d + 3 * r] = dt.to(dev, BF)
    ext_before = bits(DX[:, d:])
    grad = dA0.to(dev).float()
    engine._lora_qkv_input_grads(X1, DX, _lora_state(r, a_bf16=A.to(dev, BF), grad=grad), 0, d)
    assert torch.equal(grad.cpu().double(), dA0 + dt.T @ x1)
    assert torch.equal(DX[:, :d].float().cpu().double(), dx + dt @ A)
    assert torch.equal(bits(DX[:, d:]), ext_before)


# ------------------------------------------------------------------ 4. lora_pack_b / lora_pack_bt
@pytest.mark.parametrize("n,r", [(3, 16), (1, 16), (4, 16), (3, 5)])
def test_lora_pack_exact(dev, n, r):
    """(alpha / r) B into the 64 K-extension columns of the packed weight and of its transpose; d_out = 200 (n = 3: 3 * 200 * 64 = 38 400
    elements = 150 blocks of 256; n = 1: 50 blocks), scale = 2^-2, Bcat bf16-representable -> exact.  (4, 16) is the
    n * r = 64 boundary: every extension column is owned.  Everything outside adapter j's columns [j r, (j+1) r) is +0 and
    the base columns / rows keep their sentinel."""
    from vt355 import ops
    d_out, K, scale = 200, 64, 0.25
    N = n * d_out
    g = torch.Generator().manual_seed(10 * n + r)
    Bc = rb(torch.randn(N, r, generator=g))
    ref = torch.zeros(N, 64)
    for j in range(n):
        ref[j * d_out:(j + 1) * d_out, j * r:(j + 1) * r] = scale * Bc[j * d_out:(j + 1) * d_out]
    W = torch.full((N, K + 64), SENT, dtype=BF, device=dev)
    ops.lora_pack_b(Bc.to(dev), W[:, K:], K + 64, n, d_out, r, scale)
    assert torch.equal(bits(W[:, K:]), bits(ref.to(BF))) and (W[:, :K] == SENT).all()
    WT = torch.full((K + 64, N), SENT, dtype=BF, device=dev)
    ops.lora_pack_bt(Bc.to(dev), WT[K:], N, n, d_out, r, scale)
    assert torch.equal(bits(WT[K:]), bits(ref.T.to(BF))) and (WT[:K] == SENT).all()


def test_lora_pack_refuses_more_than_64_columns(dev):
    """n * r = 5 * 13 = 65 does not fit the 64-column extension: ops.check raises VtError (a RuntimeError), nothing is written"""
    from vt355 import ops
    from vt355._lib import VtError
    Bc = torch.zeros(5 * 8, 13, device=dev)
    W = torch.full((5 * 8, 128), SENT, dtype=BF, device=dev)
    with pytest.raises(VtError, match="vt_lora_pack_b"):
        ops.lora_pack_b(Bc, W[:, 64:], 128, 5, 8, 13, 0.25)
    with pytest.raises(VtError, match="vt_lora_pack_bt"):
        ops.lora_pack_bt(Bc, W.view(128, 40)[64:], 40, 5, 8, 13, 0.25)
    assert (W == SENT).all()


# ================================================================== B. csrc/reduce.hip
# ------------------------------------------------------------------ 5. small_linear_bwd
@pytest.mark.parametrize("with_dx", [True, False], ids=["dW_db_dx", "dx_None"])
@pytest.mark.parametrize("N,K", [(40, 300), (6 * 128 + 5, 512), (16, 256)])
@pytest.mark.parametrize("Bn", [1, 2, 8])
def test_small_linear_bwd_exact(dev, Bn, N, K, with_dx):
    """dW += dy^T x, db += sum_b dy, dx += dy W on integers in {-2..2}: |dW|, |db| <= 4 * 8, |dx| <= 4 * 773 on top of integer
    start values (the contract is +=) -- exact.  Grid = (ceil(N / 16), ceil(K / 256)): N = 40 is 2 full 16-row blocks + 8 rows,
    N = 773 is 48 blocks + 5 rows, K = 300 is one full 256-column block + 44 columns; (16, 256) is exactly one block.  dx is
    summed with atomics over the N / 16 row blocks; db is written by the blockIdx.y == 0 blocks only (K = 512: not twice).
    dy (fp32) and x (bf16) are row-strided views with NaN padding, dx a strided view whose padding keeps its sentinel.
    Both argument combinations of the callers: all three outputs, and dx = None (the first Linear of the time-embedding MLP)."""
    from vt355 import ops
    g = torch.Generator().manual_seed(1000 * Bn + N + K)
    dy, x, W = ints(g, -2, 2, Bn, N), ints(g, -2, 2, Bn, K), ints(g, -2, 2, N, K)
    dW0, db0, dx0 = ints(g, 1, 5, N, K), ints(g, 1, 5, N), ints(g, 1, 5, Bn, K)
    DY = torch.full((Bn, N + 7), NAN, device=dev); DY[:, :N] = dy.to(dev).float()
    X = torch.full((Bn, K + 8), NAN, dtype=BF, device=dev); X[:, :K] = x.to(dev, BF)
    dW, db = dW0.to(dev).float(), db0.to(dev).float()
    dxbuf = torch.full((Bn, K + 5), SENT, device=dev); dxbuf[:, :K] = dx0.to(dev).float()
    ops.small_linear_bwd(DY[:, :N], X[:, :K], W.to(dev, BF), dW, db, dxbuf[:, :K] if with_dx else None)
    assert torch.equal(dW.cpu().double(), dW0 + dy.T @ x)
    assert torch.equal(db.cpu().double(), db0 + dy.sum(0))
    assert torch.equal(dxbuf[:, :K].cpu().double(), dx0 + dy @ W if with_dx else dx0)
    assert (dxbuf[:, K:] == SENT).all()


def test_small_linear_bwd_refuses_more_than_8_rows(dev):
    from vt355 import ops
    from vt355._lib import VtError
    dW = torch.zeros(16, 256, device=dev)
    with pytest.raises(VtError, match="vt_small_linear_bwd"):
        ops.small_linear_bwd(torch.ones(9, 16, device=dev), torch.ones(9, 256, dtype=BF, device=dev),
                             torch.ones(16, 256, dtype=BF, device=dev), dW, None, None)
    assert (dW == 0).all()


# ------------------------------------------------------------------ 6. silu_bwd, silu, cast_f32_bf16
EDGES = [30.0, -30.0, 0.0, 0.0078125, -0.0078125, 88.0, -88.0, 100.0, -100.0]      # all exact in bf16


def _act_input(n, seed):
    """randn * 3 with the edge values at the END (the partial last block of n = 70 001 = 273 * 256 + 113)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * 3
    k = min(n, len(EDGES))
    x[n - k:] = torch.tensor(EDGES[:k])
    return rb(x)


@pytest.mark.parametrize("n", [1, 70001])
def test_silu_bwd(dev, n):
    """dx = dy * silu'(x), fp32 out, x bf16 pre-activation; fp64 reference on the same bf16 input.  Bar: this suite's fp32 bar
    (test_kernels_gpu.py header, 1e-4) -- rtol 1e-4 / atol 1e-5 * max|dy|.  n = 70 001 is 274 blocks with 113 threads in the last.
    Finite everywhere (exp(88), exp(100) overflow or nearly so); at x = -100 the result is exactly +-0, at +100 exactly dy.
    The output starts as NaN (the kernel overwrites) and the element after the n-th keeps its sentinel."""
    from vt355 import ops
    x = _act_input(n, 6)
    g = torch.Generator().manual_seed(n)
    dy = torch.randn(n, generator=g)
    s = torch.sigmoid(x.double())
    ref = dy.double() * (s * (1 + x.double() * (1 - s)))
    out = torch.full((n + 3,), NAN, device=dev); out[n:] = SENT
    ops.silu_bwd(dy.to(dev), x.to(dev, BF), out[:n])
    got = out.cpu()
    assert torch.isfinite(got).all() and (got[n:] == SENT).all()
    close(got[:n], ref, 1e-4, 1e-5 * dy.abs().max().item(), "silu_bwd")
    if n > 1:
        assert x[n - 1] == -100 and got[n - 1] == 0.0
        assert x[n - 2] == 100 and got[n - 2] == dy[n - 2]


@pytest.mark.parametrize("n", [1, 70001])
def test_silu(dev, n):
    """y = x * sigmoid(x), bf16 in and out, against fp64 on the same input; bar rtol 1e-2 / atol 1e-3 (bf16 storage: 2^-9 relative)"""
    from vt355 import ops
    x = _act_input(n, 7)
    out = torch.full((n + 3,), SENT, dtype=BF, device=dev)
    ops.silu(x.to(dev, BF), out[:n])
    got = out.float().cpu()
    assert torch.isfinite(got).all() and (got[n:] == SENT).all()
    close(got[:n], x.double() * torch.sigmoid(x.double()), 1e-2, 1e-3, "silu")


@pytest.mark.parametrize("n", [1, 70001, 2 * 2097152 + 77])
def test_cast_f32_bf16_is_round_to_nearest_even(dev, n):
    """bit for bit x.to(bfloat16): randn * 3 and the edge values; 4000 exact ties (low half 0x8000 under random even and odd
    upper halves over the whole normal range, both signs); their neighbours 0x7FFF / 0x8001; and values that round up into the
    next binade (upper half 0x..7F / 0x..FF with the low half >= 0x8000, e.g. 0x3FFFFFFF -> 2.0).
    n = 2 * 2097152 + 77 is two sweeps of the capped grid (8192 workgroups x 256 threads) and 77 elements of a third."""
    from vt355 import ops
    x = _act_input(n, 8)
    g = torch.Generator().manual_seed(80)
    k = max(n - len(EDGES), 0)
    x[:k] = torch.randn(k, generator=g) * 3                        # NOT pre-rounded: the low 16 bits are random
    if n == 1:
        x[0] = 1.00390625 + 2.0 ** -20                             # just above the tie between 1.0 and 1.0078125
    if n > 8000:
        g = torch.Generator().manual_seed(9)
        hi = torch.randint(0x0080, 0x7F00, (4000,), generator=g) | (torch.randint(0, 2, (4000,), generator=g) << 15)
        tie = (hi << 16) | 0x8000
        carry = ((hi | 0x7F) << 16) | torch.randint(0x8000, 0x10000, (4000,), generator=g)
        special = torch.cat([tie, tie - 1, tie + 1, carry, torch.tensor([0x3FFFFFFF, 0x3F808000, 0x3F818000, 0x3FFF8000])])
        special = torch.from_numpy(special.numpy().astype(np.uint32).view(np.float32).copy())
        assert torch.isfinite(special).all()
        x[100:100 + special.numel()] = special
    out = torch.full((n + 3,), SENT, dtype=BF, device=dev)
    ops.cast_f32_bf16(x.to(dev), out[:n])
    assert torch.equal(bits(out[:n]), bits(x.to(BF))) and (out[n:] == SENT).all()


# ------------------------------------------------------------------ 7. ln_param_combine
def _bounded(got, ref, mag, what):
    """|got - ref| <= 2^-20 * (sum of the |terms| of the element), ref and mag in fp64"""
    err = (got.double().cpu() - ref).abs()
    bad = ~(err <= 2.0 ** -20 * mag)
    assert not bad.any(), f"{what}: {bad.sum().item()} elements past the bound, worst ratio {(err / (2.0 ** -20 * mag)).max().item():.3g}"


@pytest.mark.parametrize("D", [64, 300])
def test_ln_param_combine_alone(dev, D):
    """random fp32 G1 / G2, B = 3; D = 64 is a quarter block, D = 300 a full 256-thread block + 44.  Outputs are pre-filled (+=).
    Every output element is a sum of at most G + 1 fp32 products (its start value and one or two products per group), each
    rounded a few times at 2^-24 relative: the error is bounded by 2^-20 * sum |terms| (derived, not measured; the sum of the
    magnitudes is formed in fp64 here).
      grouped: G = 2B groups (text, video per sample), txt / vid scales and all four dmods slices inside ONE [B, nmod] table laid
        out by engine._mod, as engine_fullft does; the table's other entries (gates, the neighbouring LayerNorm) are untouched.
      ungrouped: G = 1 (row 1 of the scratch, as the norm_final call), scales = None, dmods = None: dgamma += G2, dbeta += G1 exactly.
      dgamma = None: only the modulation gradients are written."""
    from vt355 import engine, ops
    B = 3
    g = torch.Generator().manual_seed(D)
    G1, G2 = torch.randn(2 * B, D, generator=g) * 5, torch.randn(2 * B, D, generator=g) * 5
    gam, bet = rb(1 + 0.2 * torch.randn(D, generator=g)), rb(0.2 * torch.randn(D, generator=g))
    nmod = 2 * 6 * D + 2 * D
    mod = torch.randn(B, nmod, generator=g) * 0.3
    dmod0 = torch.randn(B, nmod, generator=g)
    dg0, db0 = torch.randn(D, generator=g), torch.randn(D, generator=g)
    G1d, G2d, gd, bd, modd = G1.to(dev), G2.to(dev), gam.to(dev, BF), bet.to(dev, BF), mod.to(dev)
    m = engine._mod(modd, 1, D)
    o = 6 * D                                                   # LayerNormZero number 1 of the table
    sc = torch.stack([mod[:, o + 4 * D:o + 5 * D], mod[:, o + D:o + 2 * D]], 1).reshape(2 * B, D).double()      # group 2b + seg: text, video
    g1, g2, ga, be = G1.double(), G2.double(), gam.double(), bet.double()

    def mod_refs():
        ref, mag = dmod0.double().clone(), dmod0.double().abs()
        for b in range(B):
            for seg, k_shift, k_scale in ((0, 3, 4), (1, 0, 1)):
                r1, r2 = g1[2 * b + seg], g2[2 * b + seg]
                ref[b, o + k_shift * D:o + (k_shift + 1) * D] += r1
                mag[b, o + k_shift * D:o + (k_shift + 1) * D] += r1.abs()
                ref[b, o + k_scale * D:o + (k_scale + 1) * D] += ga * r2 + be * r1
                mag[b, o + k_scale * D:o + (k_scale + 1) * D] += (ga * r2).abs() + (be * r1).abs()
        return ref, mag
    touched = torch.zeros(nmod, dtype=torch.bool)
    for k in (0, 1, 3, 4):
        touched[o + k * D:o + (k + 1) * D] = True

    for with_gamma in (True, False):
        dmod = dmod0.clone().to(dev); dm = engine._mod(dmod, 1, D)
        dg, db = dg0.clone().to(dev), db0.clone().to(dev)
        ops.ln_param_combine(G1d, G2d, D, gd, bd, (m.scale_txt, m.scale_vid, m.bs), dg if with_gamma else None, db if with_gamma else None,
                             (dm.shift_txt, dm.shift_vid, dm.scale_txt, dm.scale_vid, nmod), True)
        ref, mag = mod_refs()
        _bounded(dmod, ref, mag, "dshift / dscale")
        assert torch.equal(dmod.cpu()[:, ~touched], dmod0[:, ~touched]), "wrote outside the four modulation slices"
        if with_gamma:
            _bounded(dg, dg0.double() + ((1 + sc) * g2).sum(0), dg0.double().abs() + ((1 + sc) * g2).abs().sum(0), "dgamma")
            _bounded(db, db0.double() + ((1 + sc) * g1).sum(0), db0.double().abs() + ((1 + sc) * g1).abs().sum(0), "dbeta")
        else:
            assert torch.equal(dg.cpu(), dg0) and torch.equal(db.cpu(), db0)

    dg, db = dg0.clone().to(dev), db0.clone().to(dev)
    ops.ln_param_combine(G1d[1:2], G2d[1:2], D, gd, bd, None, dg, db, None, False)
    assert torch.equal(dg.cpu(), dg0 + G2[1]) and torch.equal(db.cpu(), db0 + G1[1])        # one fp32 add each: correctly rounded


def test_ln_param_chain_vs_autograd(dev):
    """ln_modulate_fwd -> group_colsum(grouped) -> ln_param_combine, the chain engine_fullft.ln_grads runs, at B = 2, S = 301,
    St = 17, D = 192, against fp64 autograd of cogvideox_oracle.ln_modulate w.r.t. gamma, beta and the per-sample text / video
    shift and scale.  Bar: rtol 1e-4, atol 3e-3 * max|ref| -- the one test_group_colsum_* set for these sums."""
    from vt355 import engine, ops
    B, S, St, D = 2, 301, 17, 192
    M = B * S
    g = torch.Generator().manual_seed(73)
    x = rb(torch.randn(M, D, generator=g) * 2 + 0.5); dy = rb(torch.randn(M, D, generator=g))
    gam, bet = rb(1 + 0.1 * torch.randn(D, generator=g)), rb(0.1 * torch.randn(D, generator=g))
    mod = torch.randn(B, 6 * D, generator=g) * 0.3
    ga, be, mo = [t.double().requires_grad_(True) for t in (gam, bet, mod)]
    rows_b = torch.arange(M) // S
    is_txt = ((torch.arange(M) % S) < St)[:, None]
    shift = torch.where(is_txt, mo[rows_b, 3 * D:4 * D], mo[rows_b, 0:D])
    scale = torch.where(is_txt, mo[rows_b, 4 * D:5 * D], mo[rows_b, D:2 * D])
    O.ln_modulate(x.double(), ga, be, scale, shift, 1e-5).backward(dy.double())

    X, DY, Y = x.to(dev, BF), dy.to(dev, BF), poisoned((M, D), BF, dev)
    mean, rstd = poisoned((M,), torch.float32, dev), poisoned((M,), torch.float32, dev)
    modd = mod.to(dev); m = engine._mod(modd, 0, D)
    gd, bd = gam.to(dev, BF), bet.to(dev, BF)
    ops.ln_modulate_fwd(X, Y, gd, bd, (m.shift_txt, m.scale_txt, m.shift_vid, m.scale_vid, m.bs), mean, rstd, D, S, St, 1e-5)
    G1, G2 = torch.zeros(2 * B, D, device=dev), torch.zeros(2 * B, D, device=dev)
    ops.group_colsum(DY, G1, y=X, out2=G2, mean=mean, rstd=rstd, D=D, S=S, St=St, grouped=True)
    dmod = torch.zeros(B, 6 * D, device=dev); dm = engine._mod(dmod, 0, D)
    dg, db = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    ops.ln_param_combine(G1, G2, D, gd, bd, (m.scale_txt, m.scale_vid, m.bs), dg, db,
                         (dm.shift_txt, dm.shift_vid, dm.scale_txt, dm.scale_vid, 6 * D), True)
    close(dg, ga.grad, 1e-4, 3e-3 * ga.grad.abs().max().item(), "dgamma")
    close(db, be.grad, 1e-4, 3e-3 * be.grad.abs().max().item(), "dbeta")
    for k, name in ((0, "dshift_vid"), (1, "dscale_vid"), (3, "dshift_txt"), (4, "dscale_txt")):
        ref = mo.grad[:, k * D:(k + 1) * D]
        close(dmod[:, k * D:(k + 1) * D], ref, 1e-4, 3e-3 * ref.abs().max().item(), name)
    for k in (2, 5):                                              # the gate slots belong to another kernel
        assert (dmod[:, k * D:(k + 1) * D] == 0).all()


# ------------------------------------------------------------------ 8. qk_ln_param_grads
@pytest.mark.parametrize("with_rope", [False, True], ids=["plain", "rope"])
def test_qk_ln_param_grads(dev, with_rope):
    """per-head LayerNorm(64) gamma / beta gradients of q and k at M = 4100, H = 4: M * 2H = 32 800 groups against the 1024-block
    cap x 32 groups = 32 768, so 32 groups take a second trip of the stride loop.  out [2, 2, 64] starts non-zero (+=).
    dq_hat is an integer-valued fp32 view with a row stride of H * 64 + 8 (NaN padding), dk_hat integer-valued bf16.
    Without RoPE the two beta rows are integer column sums (|sum| <= 2 * 16 400): torch.equal.  The gamma rows (and, with the
    golden rotary tables of tests/golden/rope_3d.npz on S = 100 = 40 text + 60 video rows, 41 samples, all four rows) get
    rtol 1e-4 / atol 3e-3 * max|ref| against fp64 with the device's own mean / rstd from qk_layernorm_fwd."""
    from vt355 import ops
    M, H = 4100, 4
    D = H * 64
    g = torch.Generator().manual_seed(41)
    qkv = rb(torch.randn(M, 3 * D, generator=g) * 1.5)
    prm = [rb(t) for t in (1 + 0.2 * torch.randn(64, generator=g), 0.2 * torch.randn(64, generator=g),
                           1 + 0.2 * torch.randn(64, generator=g), 0.2 * torch.randn(64, generator=g))]
    dq, dk = ints(g, -2, 2, M, D), ints(g, -2, 2, M, D)
    out0 = ints(g, 1, 5, 2, 2, 64)
    rope, S, St = None, M, M
    if with_rope:
        gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "rope_3d.npz"))
        cos, sin = torch.from_numpy(gold["small_cos"]), torch.from_numpy(gold["small_sin"])     # [60, 64]
        S, St = 100, 40
        rope = (cos.to(dev).contiguous(), sin.to(dev).contiguous(), S, St)
    Q = qkv.to(dev, BF); qk_hat = poisoned((M, 2 * D), BF, dev)
    mean = poisoned((M, 2 * H), torch.float32, dev); rstd = poisoned((M, 2 * H), torch.float32, dev)
    pd = [t.to(dev, BF) for t in prm]
    ops.qk_layernorm_fwd(Q, qk_hat, pd[0], pd[1], pd[2], pd[3], mean, rstd, H, 1e-6, rope=rope)
    DQ = torch.full((M, D + 8), NAN, device=dev); DQ[:, :D] = dq.to(dev).float()
    out = out0.to(dev).float()
    ops.qk_ln_param_grads(DQ[:, :D], dk.to(dev, BF), Q, mean, rstd, out, H, rope=rope)
    got = out.cpu().double() - out0

    mu, rs = mean.cpu().double(), rstd.cpu().double()
    for w, dy in ((0, dq), (1, dk)):
        xhat = (qkv[:, w * D:(w + 1) * D].double().view(M, H, 64) - mu[:, w * H:(w + 1) * H, None]) * rs[:, w * H:(w + 1) * H, None]
        dy = dy.view(M, H, 64)
        if not with_rope:
            ref_g, ref_b = (dy * xhat).sum((0, 1)), dy.sum((0, 1))
            assert torch.equal(got[w, 1], ref_b), f"beta row {w}: {(got[w, 1] != ref_b).sum().item()} of 64 differ"
        else:
            ga, be = torch.ones(64, dtype=torch.float64, requires_grad=True), torch.zeros(64, dtype=torch.float64, requires_grad=True)
            y = (xhat * ga + be).view(M // S, S, H, 64).transpose(1, 2)                       # [B, H, S, 64]
            y = torch.cat([y[:, :, :St], O.apply_rope(y[:, :, St:], cos.double(), sin.double())], dim=2)
            (y * dy.view(M // S, S, H, 64).transpose(1, 2)).sum().backward()
            ref_g, ref_b = ga.grad, be.grad
            close(got[w, 1], ref_b, 1e-4, 3e-3 * ref_b.abs().max().item(), f"rope beta row {w}")
        close(got[w, 0], ref_g, 1e-4, 3e-3 * ref_g.abs().max().item(), f"gamma row {w}")


# ================================================================== C. csrc/elementwise.hip
# ------------------------------------------------------------------ 9. diffusion_loss with dvpred, diffusion_loss_bwd
@functools.lru_cache(maxsize=None)
def _loss_data():
    B, per = 3, 50001
    g = torch.Generator().manual_seed(50)
    abar = O.alphas_cumprod_cogvideox()
    t = torch.tensor([10, 500, 990])
    sa, sb, w = abar[t].sqrt().float(), (1 - abar[t]).sqrt().float(), (1 / (1 - abar[t])).float()
    x0 = torch.randn(B, per, generator=g)
    noisy, v = rb(torch.randn(B, per, generator=g)), rb(torch.randn(B, per, generator=g))
    vv = v.double().requires_grad_(True)
    pred = sa.double()[:, None] * noisy.double() - sb.double()[:, None] * vv
    loss = (w.double()[:, None] * (pred - x0.double()) ** 2).mean(1).mean()
    loss.backward()
    return sa, sb, w, x0, noisy, v, loss.detach(), vv.grad


@pytest.mark.parametrize("grad_out", [1.0, 0.37])
def test_diffusion_loss_and_bwd(dev, grad_out):
    """B = 3, per = 50 001: 150 003 elements against the fixed grid of 512 blocks x 256 = 131 072 threads, so 18 931 threads take
    a second trip of the stride loop; the sample boundaries (50 001, 100 002) are no multiples of 256.  Timesteps {10, 500, 990}.
    vt_diffusion_loss (loss + dvpred, host grad_scale) and vt_diffusion_loss_bwd (upstream gradient read from device memory) must
    give the same bits when grad_scale == grad_out; both against fp64 autograd at the existing bars of test_noise_loss_adamw:
    gradient rtol 1e-2 / atol 1e-2 * max|ref|, loss rtol 1e-4 / atol 1e-5.  The bf16 element after the last keeps its sentinel."""
    from vt355 import ops
    sa, sb, w, x0, noisy, v, loss_ref, dv_ref = _loss_data()
    B, per = x0.shape
    n = B * per
    dv_ref = dv_ref * grad_out
    args = (v.to(dev, BF), noisy.to(dev, BF), x0.to(dev), sa.to(dev), sb.to(dev), w.to(dev))
    loss = poisoned((1,), torch.float32, dev); part = poisoned((512,), torch.float32, dev)
    dv1 = torch.full((n + 3,), SENT, dtype=BF, device=dev); dv2 = dv1.clone()
    ops.diffusion_loss(*args, loss, part, dv1[:n].view(B, per), grad_out)
    ops.diffusion_loss_bwd(*args, torch.tensor([grad_out], device=dev), dv2[:n].view(B, per))
    close(loss, loss_ref.reshape(1), 1e-4, 1e-5, "loss")
    atol = 1e-2 * dv_ref.abs().max().item()
    close(dv1[:n].view(B, per), dv_ref, 1e-2, atol, "dvpred of diffusion_loss")
    close(dv2[:n].view(B, per), dv_ref, 1e-2, atol, "dvpred of diffusion_loss_bwd")
    assert torch.equal(bits(dv1), bits(dv2)), "the two kernels disagree"
    assert (dv1[n:] == SENT).all()
