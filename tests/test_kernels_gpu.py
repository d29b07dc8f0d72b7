"""Per-kernel parity: every HIP entry point (called through the C-ABI) against the CPU oracle / a plain
fp32 PyTorch restatement of the same op on the same seeded inputs.  Tolerances are bf16-storage
tolerances (8 significant bits): outputs are compared with rtol/atol ~1-2e-2 against an fp32 reference fed
with the SAME bf16-rounded inputs; fp32 outputs (LSE, statistics, loss, AdamW) use 1e-4..1e-3."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cogvideox_oracle as O
from parity import close, poisoned, poisoned_like, untouched

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def rb(x):      # bf16-round but keep fp32 (what the device kernel actually sees)
    return x.to(BF).float()


# ------------------------------------------------------------------ GEMM
@pytest.fixture(params=[1, 2, 3], ids=["tile128", "tile256", "tile256x128_pc"])
def gemm_tile(request):
    """both tilings of vt_gemm_bf16 (the library picks by shape; the tests force each one on every shape)"""
    from vt355 import ops
    ops.gemm_set_tile(request.param)
    yield request.param
    ops.gemm_set_tile(0)


@pytest.mark.parametrize("M,N,K", [(300, 256, 128), (1000, 1984, 1920), (129, 128, 64), (2, 1536, 512), (17776, 1920, 1984),
                                   (513, 772, 192)])
def test_gemm_bias(dev, M, N, K, gemm_tile):
    from vt355 import ops
    g = torch.Generator().manual_seed(M + N + K)
    a = rb(torch.randn(M, K, generator=g)); w = rb(torch.randn(N, K, generator=g) * 0.05); b = rb(torch.randn(N, generator=g))
    ref = a @ w.T + b
    out = poisoned((M, N), BF, dev)
    ops.gemm(a.to(dev, BF), w.to(dev, BF), out, b.to(dev, BF))
    close(out, ref, 1e-2, 1e-2, "gemm bf16 out")
    out32 = poisoned((M, N), torch.float32, dev)
    ops.gemm(a.to(dev, BF), w.to(dev, BF), out32, b.to(dev, BF))
    close(out32, ref, 1e-4, 2e-3, "gemm fp32 out")


@pytest.mark.parametrize("N", [256, 388])
@pytest.mark.parametrize("B,S,St", [(2, 150, 20), (3, 300, 37)], ids=["S150", "S300"])     # S300: a 256-row tile spans two samples
def test_gemm_strided_and_epilogues(dev, gemm_tile, N, B, S, St):
    from vt355 import ops
    g = torch.Generator().manual_seed(7)
    K = 128
    M = B * S
    abig = rb(torch.randn(M, K + 64, generator=g))            # lda > K (extension columns ignored via K=)
    w = rb(torch.randn(N, K, generator=g) * 0.1); bias = rb(torch.randn(N, generator=g))
    a = abig[:, :K]
    A = abig.to(dev, BF); W = w.to(dev, BF); Bi = bias.to(dev, BF)
    # GELU epilogue: two outputs
    u_ref = a @ w.T + bias
    out = poisoned((M, N), BF, dev); pre = poisoned((M, N), BF, dev)
    ops.gemm(A, W, out, Bi, epilogue=ops.EPI_BIAS_GELU, pre_act_out=pre, K=K)
    close(pre, u_ref, 1e-2, 1e-2, "pre-activation")
    close(out, F.gelu(u_ref, approximate="tanh"), 1e-2, 1e-2, "gelu")
    # gated residual, text/video gates per sample
    R = rb(torch.randn(M, N, generator=g)); gates = torch.randn(B, 2, N, generator=g)
    gate_rows = torch.stack([gates[m // S, 0 if (m % S) < St else 1] for m in range(M)])
    ref = R + gate_rows * u_ref
    G = gates.to(dev)
    out = poisoned((M, N), BF, dev)            # a fresh poisoned output per epilogue: the previous one's values are not evidence
    ops.gemm(A, W, out, Bi, epilogue=ops.EPI_GATED_RES, residual=R.to(dev, BF), gate_txt=G[:, 0], gate_vid=G[:, 1],
             gate_bstride=2 * N, S=S, St=St, K=K)
    close(out, ref, 1e-2, 2e-2, "gated residual")
    # positional-table add (gate None, r_mod)
    tab = rb(torch.randn(S, N, generator=g))
    out = poisoned((M, N), BF, dev)
    ops.gemm(A, W, out, Bi, epilogue=ops.EPI_GATED_RES, residual=tab.to(dev, BF), r_mod=S, K=K)
    close(out, tab.repeat(B, 1) + u_ref, 1e-2, 2e-2, "pos add")
    # dGELU
    U = rb(torch.randn(M, N, generator=g))
    uu = U.clone().requires_grad_(True)
    F.gelu(uu, approximate="tanh").sum().backward()
    out = poisoned((M, N), BF, dev)
    ops.gemm(A, W, out, None, epilogue=ops.EPI_DGELU, pre_act_in=U.to(dev, BF), K=K)
    close(out, (a @ w.T) * uu.grad, 1e-2, 2e-2, "dgelu")


# ------------------------------------------------------------------ attention
def _qkv(B, S, H, g, spike=False):
    qkv = torch.randn(B, S, 3, H, 64, generator=g)
    if spike:
        qkv[:, S // 2, 1] *= 6.0        # one key row much larger: forces the running max to jump mid-stream
        qkv[:, 3, 0] *= 4.0
    return rb(qkv)


SC2 = math.log2(math.e) / 8.0


def _prescale(qkv, pre):
    """device copy of qkv (q multiplied by scale*log2e and re-rounded when pre) + the exact q the kernel then sees."""
    if not pre:
        return qkv, qkv
    dq = qkv.clone()
    dq[:, :, 0] = rb(qkv[:, :, 0] * SC2)
    ref = qkv.double().clone()
    ref[:, :, 0] = dq[:, :, 0].double() / SC2
    return dq, ref


@pytest.mark.parametrize("pre", [False, True, "tiles16"])
@pytest.mark.parametrize("B,S,H,spike", [(1, 64, 1, False), (2, 100, 2, False), (1, 333, 3, True), (1, 1250, 2, False)])
def test_attn_fwd(dev, B, S, H, spike, pre):
    """pre = "tiles16": the 16x16x32-MFMA variant of the pre-scaled forward (not the default: slower inside the training step)"""
    from vt355 import ops
    tiles16 = pre == "tiles16"
    pre = bool(pre)
    g = torch.Generator().manual_seed(S)
    qkv = _qkv(B, S, H, g, spike)
    qkv_dev, qkv_ref = _prescale(qkv, pre)
    q, k, v = [qkv_ref[:, :, i].permute(0, 2, 1, 3).double() for i in range(3)]
    o_ref, lse_ref = O.attention(q, k, v)
    d = qkv_dev.to(dev, BF).view(B, S, 3 * H * 64)
    o = poisoned((B, S, H * 64), BF, dev)
    lse2 = poisoned((B, H, S), torch.float32, dev)
    ops.attn_fwd(d[:, :, :H * 64], d[:, :, H * 64:2 * H * 64], d[:, :, 2 * H * 64:], o, lse2, B, H, S, q_prescaled=pre, tiles16=tiles16)
    close(o.view(B, S, H, 64).permute(0, 2, 1, 3), o_ref, 2e-2, 1e-2, "attn out")
    close(lse2 * math.log(2.0), lse_ref, 1e-4, 2e-3, "lse")


@pytest.mark.parametrize("chain", [0, 1, 2], ids=["atomics", "chains", "chains_3gen"])
@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("B,S,H,spike", [(1, 64, 1, False), (2, 100, 2, False), (1, 333, 3, True), (1, 700, 2, False), (1, 256, 1, False),
                                         (1, 3000, 2, False), (2, 2700, 3, True)])
def test_attn_bwd(dev, B, S, H, spike, pre, chain):
    """chain 0: no workspace, every key block adds its dQ atomically.  chain 1: with the workspace; in the two long cases (12 / 11 key blocks
    per head) runs of consecutive key blocks hand their dQ tiles to each other: chains of 3 (the default length), cut at head ends and XCD
    slot-range ends.  The cases with S <= 700 have at most 8 workgroups, the chain length is clamped to grid / 8 = 1 and they run the
    atomics path although a workspace is given (vt_attn_bwd_chain_plan says so below; tests/test_attn64_gpu.py has the small shapes that
    do chain).  chain 2: the long cases on a 24-slot grid -> several generations per slot, chains of 3, slots that change role between
    generations."""
    if S > 1000 and not pre:
        pytest.skip("long cases run once (prescaled, the engine's configuration)")
    if chain == 2 and S < 1000:
        pytest.skip("multi-generation case needs more key blocks than slots")
    from vt355 import ops
    ops.attn_bwd_set_chain(0, 24 if chain == 2 else 0)
    g = torch.Generator().manual_seed(S + 1)
    qkv = _qkv(B, S, H, g, spike)
    qkv, qkv_ref = _prescale(qkv, pre)
    do = rb(torch.randn(B, S, H, 64, generator=g))
    qkv64 = qkv_ref.double().requires_grad_(True)
    q, k, v = [qkv64[:, :, i].permute(0, 2, 1, 3) for i in range(3)]
    o_ref, _ = O.attention(q, k, v)
    o_ref.backward(do.permute(0, 2, 1, 3).double())
    dref = qkv64.grad                                   # [B,S,3,H,64]
    d = qkv.to(dev, BF).view(B, S, 3 * H * 64)
    D = H * 64
    qd, kd, vd = d[:, :, :D], d[:, :, D:2 * D], d[:, :, 2 * D:]
    o = poisoned((B, S, D), BF, dev); lse2 = poisoned((B, H, S), torch.float32, dev)
    ops.attn_fwd(qd, kd, vd, o, lse2, B, H, S, q_prescaled=pre)
    dq = torch.zeros(B, S, D, dtype=torch.float32, device=dev)               # in/out: fp32 atomics accumulate into it
    dk = poisoned((B, S, D), BF, dev); dv = poisoned((B, S, D), BF, dev)      # written whole
    delta = poisoned((B * H * S,), torch.float32, dev)             # scratch: written by the first pass before it is read
    ws = ops.attn_bwd_chain_workspace(B, H, S, dev) if chain else None
    assert (ws is not None) == bool(chain)
    try:
        planned = ops.attn_bwd_chain_plan(B, H, S, have_ws=ws is not None)[0]
        assert planned == (3 if chain and S > 1000 else 1), "the launch would not take the path this id names"
        ops.attn_bwd(qd, kd, vd, o, do.to(dev, BF).view(B, S, D), lse2, delta, dq, dk, dv, B, H, S, q_prescaled=pre, chain_ws=ws)
        if chain:
            assert ops.attn_bwd_chain_error(ws) == 0
    finally:
        ops.attn_bwd_set_chain(0, 0)
    scale = dref.abs().max().item()
    close(dq.view(B, S, H, 64), dref[:, :, 0], 3e-2, 1e-2 * scale, "dq")
    close(dk.view(B, S, H, 64), dref[:, :, 1], 3e-2, 1e-2 * scale, "dk")
    close(dv.view(B, S, H, 64), dref[:, :, 2], 3e-2, 1e-2 * scale, "dv")


def test_attn_bwd_timeout_is_sticky_and_the_optimizer_refuses_the_step(dev):
    """libvt355_test.so holds the attention backward built with CH_SPIN_LIMIT=0: every dQ hand-off wait that is not
    satisfied at once gives up.  The per-launch error word is set, the STICKY counter keeps it after a later clean launch
    of the shipped kernel on the same workspace, vt_adamw leaves parameters / moments untouched while the counter is
    non-zero, and FusedAdamW raises at the next step."""
    import ctypes as C
    import os
    from vt355 import ops, _lib
    from vt355.optim import FusedAdamW
    tpath = os.path.join(os.path.dirname(_lib.lib_path()), "libvt355_test.so")
    assert os.path.exists(tpath), "libvt355_test.so missing: run __graft_entry__.build()"
    _lib.load_library()
    tlib = C.CDLL(tpath)
    fn = tlib.vt_attn_bwd_hd64_tmo
    fn.argtypes = _lib.PROTOTYPES["vt_attn_bwd_hd64"]; fn.restype = C.c_int
    B, S, H = 1, 3000, 2
    D = H * 64
    g = torch.Generator().manual_seed(5)
    d = rb(torch.randn(B, S, 3 * D, generator=g)).to(dev, BF)
    qd, kd, vd = d[:, :, :D], d[:, :, D:2 * D], d[:, :, 2 * D:]
    o = poisoned((B, S, D), BF, dev); lse2 = poisoned((B, H, S), torch.float32, dev)
    ops.attn_fwd(qd, kd, vd, o, lse2, B, H, S)
    do = rb(torch.randn(B, S, D, generator=g)).to(dev, BF)
    dq = torch.zeros(B, S, D, dtype=torch.float32, device=dev)      # in/out: fp32 atomics accumulate into it
    dk = poisoned((B, S, D), BF, dev); dv = poisoned((B, S, D), BF, dev)
    delta = poisoned((B * H * S,), torch.float32, dev)
    ws = ops.attn_bwd_chain_workspace(B, H, S, dev)
    assert ws is not None
    ops.attn_bwd_chain_errors_clear()
    st = torch.cuda.current_stream().cuda_stream
    rc = fn(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), do.data_ptr(), lse2.data_ptr(), delta.data_ptr(),
            dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), B, H, S,
            qd.stride(1), kd.stride(1), vd.stride(1), o.stride(1), do.stride(1), dq.stride(1), dk.stride(1), dv.stride(1),
            qd.stride(0), kd.stride(0), vd.stride(0), o.stride(0), do.stride(0), dq.stride(0), dk.stride(0), dv.stride(0),
            0.125, 0, ws.data_ptr(), ws.numel(), st)
    assert rc == 0
    assert ops.attn_bwd_chain_error(ws) != 0, "the CH_SPIN_LIMIT=0 build did not time out"
    try:
        # a later clean launch clears the per-launch word but not the sticky count
        dq.zero_()
        ops.attn_bwd(qd, kd, vd, o, do, lse2, delta, dq, dk, dv, B, H, S, chain_ws=ws)
        assert ops.attn_bwd_chain_error(ws) == 0
        assert ops.attn_bwd_chain_errors() > 0
        # the optimizer refuses the update on the device and raises at the next step
        p = torch.nn.Parameter(torch.ones(1000, device=dev)); p.grad = torch.ones(1000, device=dev)
        opt = FusedAdamW([p], lr=0.1)
        opt.step()
        assert torch.all(p.detach() == 1.0) and torch.all(opt.m[0] == 0.0), "vt_adamw ran although the guard was set"
        with pytest.raises(_lib.VtError, match="timed out"):
            opt.step()
    finally:
        ops.attn_bwd_chain_errors_clear()
    opt2 = FusedAdamW([p], lr=0.1)
    opt2.step(); opt2.step()                      # cleared: the update runs again
    assert torch.all(p.detach() < 1.0)


def test_attn_bwd_timeout_is_repaired_by_redoing_the_launch_without_chains(dev):
    """default policy (VT355_CHAIN_VERIFY=launch): ops.attn_bwd reads the error word after a chained launch; when a hand-off wait timed out
    (forced here: the CH_SPIN_LIMIT=0 build of libvt355_test.so as the entry point) the launch is redone with plain atomics -- the
    gradients are the atomics-only ones, the sticky count is cleared so the optimizer takes its step, a warning is issued and the chains
    stay off for the rest of the process (restored at the end of this test)"""
    import ctypes as C
    import os
    from vt355 import ops, _lib
    from vt355.optim import FusedAdamW
    _lib.load_library()
    tlib = C.CDLL(os.path.join(os.path.dirname(_lib.lib_path()), "libvt355_test.so"))
    fn = tlib.vt_attn_bwd_hd64_tmo
    fn.argtypes = _lib.PROTOTYPES["vt_attn_bwd_hd64"]; fn.restype = C.c_int
    B, S, H = 1, 3000, 2
    D = H * 64
    g = torch.Generator().manual_seed(6)
    d = rb(torch.randn(B, S, 3 * D, generator=g)).to(dev, BF)
    qd, kd, vd = d[:, :, :D], d[:, :, D:2 * D], d[:, :, 2 * D:]
    o = poisoned((B, S, D), BF, dev); lse2 = poisoned((B, H, S), torch.float32, dev)
    ops.attn_fwd(qd, kd, vd, o, lse2, B, H, S)
    do = rb(torch.randn(B, S, D, generator=g)).to(dev, BF)
    delta = poisoned((B * H * S,), torch.float32, dev)
    # dq is in/out (fp32 atomics accumulate into zeros); dk, dv are written whole
    mk = lambda: (torch.zeros(B, S, D, dtype=torch.float32, device=dev), poisoned((B, S, D), BF, dev), poisoned((B, S, D), BF, dev))
    dq0, dk0, dv0 = mk()
    ops.attn_bwd(qd, kd, vd, o, do, lse2, delta, dq0, dk0, dv0, B, H, S, chain_ws=None)          # atomics only: the reference
    ws = ops.attn_bwd_chain_workspace(B, H, S, dev)
    assert ws is not None and ops._CHAIN_STATE["verify"] == "launch"
    ops.attn_bwd_chain_errors_clear()
    n0 = ops.attn_bwd_chain_redone()
    try:
        dq, dk, dv = mk()
        with pytest.warns(UserWarning, match="redone with plain atomics"):
            ops.attn_bwd(qd, kd, vd, o, do, lse2, delta, dq, dk, dv, B, H, S, chain_ws=ws, _entry=fn)
        assert ops.attn_bwd_chain_redone() == n0 + 1
        assert torch.equal(dk, dk0) and torch.equal(dv, dv0)
        assert (dq - dq0).abs().max().item() <= 1e-5 * dq0.abs().max().item()                 # fp32 atomics: summation order only
        assert ops.attn_bwd_chain_errors() == 0 and ops.attn_bwd_chain_error(ws) == 0
        assert ops.attn_bwd_chain_workspace(B, H, S, dev) is None                               # chains stay off
        p = torch.nn.Parameter(torch.ones(1000, device=dev)); p.grad = torch.ones(1000, device=dev)
        opt = FusedAdamW([p], lr=0.1)
        opt.step(); opt.step()                                                                  # no refusal, no raise
        assert torch.all(p.detach() < 1.0)
    finally:
        ops._CHAIN_STATE["disabled"] = False
        ops.attn_bwd_chain_errors_clear()


# ------------------------------------------------------------------ norms
def _ln_modulate_case(dev, D, B=2, S=37, St=5, affine=True, rows=None):
    """vt_ln_modulate_fwd / _bwd on a strided [M, D + 64] pair of buffers: y, mean, rstd and dx are written whole (poisoned before the
    launch), the 64 pad columns of y are never written; then the plain LayerNorm call (no modulation) when there is an affine part.
    rows: (M, D, generator) -> the bf16-representable input rows, in place of the randn ones (tests/test_conditioning_gpu.py)"""
    from vt355 import ops
    g = torch.Generator().manual_seed(D)
    M = B * S
    x = rb(torch.randn(M, D, generator=g) * 2 + 0.5)
    if rows is not None:
        x = rows(M, D, g)
    ga = rb(1 + 0.1 * torch.randn(D, generator=g)); be = rb(0.1 * torch.randn(D, generator=g))
    mod = torch.randn(B, 6 * D, generator=g) * 0.3          # shift, scale, gate, eshift, escale, egate
    rows_b = torch.arange(M) // S
    is_txt = (torch.arange(M) % S) < St
    shift = torch.where(is_txt[:, None], mod[rows_b, 3 * D:4 * D], mod[rows_b, 0:D])
    scale = torch.where(is_txt[:, None], mod[rows_b, 4 * D:5 * D], mod[rows_b, D:2 * D])
    xx = x.clone().requires_grad_(True)
    ref = O.ln_modulate(xx, ga, be, scale, shift, 1e-5) if affine else F.layer_norm(xx, (D,), None, None, 1e-5) * (1 + scale) + shift
    dy = rb(torch.randn(M, D, generator=g)); dres = rb(torch.randn(M, D, generator=g))
    ref.backward(dy)
    X = torch.zeros(M, D + 64, dtype=BF, device=dev); X[:, :D] = x.to(dev, BF)      # strided input
    Y = poisoned((M, D + 64), BF, dev)
    mean = poisoned((M,), torch.float32, dev); rstd = poisoned((M,), torch.float32, dev)
    Md = mod.to(dev)
    gad, bed = (ga.to(dev, BF), be.to(dev, BF)) if affine else (None, None)
    ops.ln_modulate_fwd(X, Y, gad, bed, (Md[:, 3 * D:], Md[:, 4 * D:], Md[:, 0:], Md[:, D:], 6 * D), mean, rstd, D, S, St, 1e-5)
    close(Y[:, :D], ref, 1e-2, 2e-2, "ln_modulate fwd")
    untouched(Y, (slice(None), slice(0, D)), "ln_modulate fwd pad columns")
    close(mean, x.mean(1), 1e-4, 1e-4, "mean")
    close(rstd, 1.0 / (x.double().var(1, unbiased=False) + 1e-5).sqrt(), 1e-4, 1e-4, "rstd")
    dx = poisoned((M, D), BF, dev)
    ops.ln_modulate_bwd(dy.to(dev, BF), X, mean, rstd, gad, (Md[:, 4 * D:], Md[:, D:], 6 * D), dres.to(dev, BF), dx, D, S, St)
    close(dx, xx.grad + dres, 2e-2, 2e-2, "ln_modulate bwd")
    if affine:
        # plain LayerNorm (no modulation, affine) == norm_final
        Y = poisoned((M, D + 64), BF, dev)
        ops.ln_modulate_fwd(X, Y, gad, bed, None, None, None, D, S, St, 1e-5)
        close(Y[:, :D], F.layer_norm(x, (D,), ga, be, 1e-5), 1e-2, 2e-2, "plain LN")
        untouched(Y, (slice(None), slice(0, D)), "plain LN pad columns")


@pytest.mark.parametrize("D", [128, 1920, 3072, 8, 512, 4096])
def test_ln_modulate(dev, D):
    """the three template branches (1 / 4 / 8 chunks of 8 elements per lane): D = 128, 1920, 3072; one chunk in one lane (D = 8), exactly
    64 chunks (D = 512, the last size of the first branch) and the limit D = 4096"""
    _ln_modulate_case(dev, D)


@pytest.mark.parametrize("D,B,S,St,affine", [(128, 1, 1, 0, True), (1920, 1, 1, 1, True), (128, 2, 37, 0, True), (1920, 2, 37, 37, True),
                                            (128, 2, 37, 5, False), (3072, 2, 37, 5, False)],
                         ids=["M1_video_row", "M1_text_row", "St0", "StS", "no_affine_D128", "no_affine_D3072"])
def test_ln_modulate_edges(dev, D, B, S, St, affine):
    """a single row (one wave of a four-row block), no text rows, only text rows, and modulation without the affine part (gamma = beta =
    None with shift / scale: the norm1 / norm2 of a block whose LayerNorm has no parameters), forward and backward"""
    _ln_modulate_case(dev, D, B, S, St, affine)


def test_ln_modulate_refuses_rows_wider_than_4096(dev):
    """D = 4104 is a multiple of 8 past the 8 chunks per lane the kernels hold in registers: refused on the host, nothing is written"""
    from vt355 import ops
    from vt355._lib import VtError
    M, D = 4, 4104
    X = torch.zeros(M, D, dtype=BF, device=dev); Y = poisoned((M, D), BF, dev)
    mean = poisoned((M,), torch.float32, dev); rstd = poisoned((M,), torch.float32, dev)
    with pytest.raises(VtError, match="vt_ln_modulate_fwd"):
        ops.ln_modulate_fwd(X, Y, None, None, None, mean, rstd, D, M, 0, 1e-5)
    with pytest.raises(VtError, match="vt_ln_modulate_bwd"):
        ops.ln_modulate_bwd(X, X, mean, rstd, None, None, None, Y, D, M, 0)
    untouched(Y, [], "refused ln_modulate: y"); untouched(mean, [], "refused ln_modulate: mean")


def test_qk_layernorm(dev):
    _qk_layernorm_case(dev)


def _qk_layernorm_case(dev, rows=None):
    """rows: (M * 3 H, 64, generator) -> the bf16-representable 64-wide head rows, in place of the randn ones (tests/test_conditioning_gpu.py)"""
    from vt355 import ops
    g = torch.Generator().manual_seed(11)
    M, H = 203, 3
    D = H * 64
    qkv = rb(torch.randn(M, 3 * D, generator=g) * 1.5)
    if rows is not None:
        qkv = rows(M * 3 * H, 64, g).view(M, 3 * D)
    gq, bq, gk, bk = [rb(t) for t in (1 + 0.2 * torch.randn(64, generator=g), 0.2 * torch.randn(64, generator=g),
                                       1 + 0.2 * torch.randn(64, generator=g), 0.2 * torch.randn(64, generator=g))]
    x = qkv.clone().requires_grad_(True)
    qh = F.layer_norm(x[:, :D].view(M, H, 64), (64,), gq, bq, 1e-6).reshape(M, D)
    kh = F.layer_norm(x[:, D:2 * D].view(M, H, 64), (64,), gk, bk, 1e-6).reshape(M, D)
    dqh = torch.randn(M, D, generator=g); dkh = rb(torch.randn(M, D, generator=g))
    (qh * dqh).sum().add((kh * dkh).sum()).backward()
    Q = qkv.to(dev, BF); out = poisoned((M, 2 * D), BF, dev)
    mean = poisoned((M, 2 * H), torch.float32, dev); rstd = poisoned((M, 2 * H), torch.float32, dev)
    dv = [t.to(dev, BF) for t in (gq, bq, gk, bk)]
    ops.qk_layernorm_fwd(Q, out, dv[0], dv[1], dv[2], dv[3], mean, rstd, H, 1e-6)
    close(out[:, :D], qh, 1e-2, 2e-2, "q_hat"); close(out[:, D:], kh, 1e-2, 2e-2, "k_hat")
    dqkv = poisoned((M, 3 * D), BF, dev)              # the q and k thirds are written whole, the v third is not this kernel's
    ops.qk_layernorm_bwd(dqh.to(dev), dkh.to(dev, BF), Q, mean, rstd, dv[0], dv[2], dqkv, H)
    close(dqkv[:, :2 * D], x.grad[:, :2 * D], 2e-2, 2e-2, "qk-LN bwd")
    untouched(dqkv, (slice(None), slice(0, 2 * D)), "qk-LN bwd: the v third")
    out = poisoned((M, 2 * D), BF, dev); mean = poisoned((M, 2 * H), torch.float32, dev); rstd = poisoned((M, 2 * H), torch.float32, dev)
    ops.qk_layernorm_fwd(Q, out, dv[0], dv[1], dv[2], dv[3], mean, rstd, H, 1e-6, q_scale=SC2)
    close(out[:, :D], qh * SC2, 1e-2, 5e-3, "q_hat prescaled"); close(out[:, D:], kh, 1e-2, 2e-2, "k_hat untouched")


def test_qk_layernorm_rope(dev):
    """qk-LayerNorm with the fused rotary embedding (CogVideoX-5B): forward, input gradient and gamma/beta gradients
    against the oracle's apply_rope on a 2-sample [text 5 | video 3x4x5] sequence; golden small tables
    (tests/golden/rope_3d.npz, the reference's SAT mixin) drive the rotation."""
    import os
    import cogvideox_oracle as O
    from vt355 import ops
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "rope_3d.npz"))
    cos, sin = torch.from_numpy(gold["small_cos"]), torch.from_numpy(gold["small_sin"])     # [60, 64]
    g = torch.Generator().manual_seed(12)
    B, St, Sv, H = 2, 5, 60, 2
    S, D = St + Sv, H * 64
    M = B * S
    qkv = rb(torch.randn(M, 3 * D, generator=g) * 1.5)
    gq, bq, gk, bk = [rb(t) for t in (1 + 0.2 * torch.randn(64, generator=g), 0.2 * torch.randn(64, generator=g),
                                       1 + 0.2 * torch.randn(64, generator=g), 0.2 * torch.randn(64, generator=g))]
    x = qkv.clone().double().requires_grad_(True)
    prm = [t.clone().double().requires_grad_(True) for t in (gq, bq, gk, bk)]

    def ref(xs, ga, be):
        y = F.layer_norm(xs.reshape(B, S, H, 64).transpose(1, 2), (64,), ga, be, 1e-6)      # [B,H,S,64]
        y = torch.cat([y[:, :, :St], O.apply_rope(y[:, :, St:], cos.double(), sin.double())], dim=2)
        return y.transpose(1, 2).reshape(M, D)
    qh, kh = ref(x[:, :D], prm[0], prm[1]), ref(x[:, D:2 * D], prm[2], prm[3])
    dqh = torch.randn(M, D, generator=g); dkh = rb(torch.randn(M, D, generator=g))
    (qh * dqh.double()).sum().add((kh * dkh.double()).sum()).backward()
    Q = qkv.to(dev, BF); out = poisoned((M, 2 * D), BF, dev)
    mean = poisoned((M, 2 * H), torch.float32, dev); rstd = poisoned((M, 2 * H), torch.float32, dev)
    dv = [t.to(dev, BF) for t in (gq, bq, gk, bk)]
    rope = (cos.to(dev).contiguous(), sin.to(dev).contiguous(), S, St)
    ops.qk_layernorm_fwd(Q, out, dv[0], dv[1], dv[2], dv[3], mean, rstd, H, 1e-6, rope=rope)
    close(out[:, :D], qh.float(), 1e-2, 2e-2, "rope q_hat"); close(out[:, D:], kh.float(), 1e-2, 2e-2, "rope k_hat")
    # text rows are untouched by the rotation: identical bits to the rope-free kernel
    out0 = poisoned_like(out)
    ops.qk_layernorm_fwd(Q, out0, dv[0], dv[1], dv[2], dv[3], mean, rstd, H, 1e-6)
    o3, o03 = out.view(B, S, 2 * D), out0.view(B, S, 2 * D)
    assert torch.equal(o3[:, :St], o03[:, :St]) and not torch.equal(o3[:, St:], o03[:, St:])
    dqkv = poisoned((M, 3 * D), BF, dev)              # the q and k thirds are written whole, the v third is not this kernel's
    ops.qk_layernorm_bwd(dqh.to(dev), dkh.to(dev, BF), Q, mean, rstd, dv[0], dv[2], dqkv, H, rope=rope)
    close(dqkv[:, :2 * D], x.grad[:, :2 * D].float(), 2e-2, 2e-2, "rope qk-LN bwd")
    untouched(dqkv, (slice(None), slice(0, 2 * D)), "rope qk-LN bwd: the v third")
    pg = torch.zeros(2, 2, 64, device=dev)                        # in/out: the parameter gradients accumulate
    ops.qk_ln_param_grads(dqh.to(dev), dkh.to(dev, BF), Q, mean, rstd, pg, H, rope=rope)
    for w in range(2):
        for gb in range(2):
            close(pg[w, gb], prm[2 * w + gb].grad.float(), 2e-2, 2e-2, f"rope qk-LN param grad {w}{gb}")
    # a bad table shape is refused on the host
    with pytest.raises(ValueError):
        ops.qk_layernorm_fwd(Q, out, dv[0], dv[1], dv[2], dv[3], mean, rstd, H, 1e-6, rope=(rope[0][:-1], rope[1][:-1], S, St))


# ------------------------------------------------------------------ elementwise
def test_timestep_embedding_golden(dev):
    from vt355 import ops
    gold = np.load(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "timestep_embedding.npz"))
    t = torch.from_numpy(gold["t"]).to(dev)
    out = poisoned((len(t), 1920), BF, dev)
    ops.timestep_embedding(t, out)
    close(out, torch.from_numpy(gold["emb1920"]), 8e-3, 8e-3, "sinusoid vs reference golden")


def test_patchify_roundtrip_and_order(dev):
    from vt355 import ops
    g = torch.Generator().manual_seed(3)
    B, Fr, C, H, W, P = 2, 3, 16, 6, 8, 2
    img = rb(torch.randn(B, Fr, C, H, W, generator=g))
    tok = poisoned((B * Fr * (H // P) * (W // P), C * P * P), BF, dev)
    ops.patchify(img.to(dev, BF), tok, P)
    # oracle order: conv2d weight flattened (c p q); tokens (t h w)
    ref = img.reshape(B, Fr, C, H // P, P, W // P, P).permute(0, 1, 3, 5, 2, 4, 6).reshape(-1, C * P * P)
    close(tok, ref, 0, 0, "patchify")
    back = poisoned((B, Fr, C, H, W), BF, dev)
    ops.unpatchify(tok, back, P)
    close(back, img, 0, 0, "unpatchify roundtrip")


def test_noise_loss_adamw(dev):
    from vt355 import ops
    g = torch.Generator().manual_seed(5)
    B, per = 3, 4 * 16 * 6 * 8
    abar = O.alphas_cumprod_cogvideox()
    t = torch.tensor([10, 500, 990])
    x0 = torch.randn(B, per, generator=g); nz = torch.randn(B, per, generator=g)
    sa = abar[t].sqrt().float(); sb = (1 - abar[t]).sqrt().float(); w = (1 / (1 - abar[t])).float()
    noisy = poisoned((B, per), BF, dev)
    ops.add_noise(x0.to(dev), nz.to(dev), sa.to(dev), sb.to(dev), noisy)
    close(noisy, O.add_noise(x0, nz, t, abar.float()), 1e-2, 1e-2, "add_noise")
    v = rb(torch.randn(B, per, generator=g)).requires_grad_(True)
    nb = noisy.float().cpu()
    pred = O.get_velocity(v, nb, t, abar.float())
    loss_ref = torch.mean((w[:, None] * (pred - x0) ** 2), dim=1).mean()
    loss_ref.backward()
    loss = poisoned((1,), torch.float32, dev); part = poisoned((512,), torch.float32, dev); dvp = poisoned((B, per), BF, dev)
    ops.diffusion_loss(v.detach().to(dev, BF), noisy, x0.to(dev), sa.to(dev), sb.to(dev), w.to(dev), loss, part, dvp, 1.0)
    close(loss, loss_ref.reshape(1), 1e-4, 1e-5, "loss")
    close(dvp, v.grad, 1e-2, 1e-2 * v.grad.abs().max().item(), "dloss/dv")
    # AdamW vs torch.optim.AdamW over 3 steps
    n = 5000
    p = torch.randn(n, generator=g); gr = [torch.randn(n, generator=g) * 0.1 for _ in range(3)]
    pt = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=1e-2)
    # in/out: the parameter and AdamW's two moments; the bf16 copy is written whole
    P = p.to(dev); Mo = torch.zeros(n, device=dev); Vo = torch.zeros(n, device=dev); Pb = poisoned((n,), BF, dev)
    for i in range(3):
        pt.grad = gr[i].clone(); opt.step()
        ops.adamw(P, gr[i].to(dev), Mo, Vo, Pb, 1e-2, 0.9, 0.999, 1e-8, 1e-2, i + 1)
    close(P, pt, 1e-5, 1e-6, "adamw")
    close(Pb, pt, 1e-2, 1e-3, "adamw bf16 copy")


# ------------------------------------------------------------------ LoRA
def test_lora_kernels(dev):
    from vt355 import ops
    g = torch.Generator().manual_seed(9)
    M, K, N, r = 333, 128, 256, 4
    x = rb(torch.randn(M, K, generator=g)); A = rb(torch.randn(12, K, generator=g) * 0.1)
    X = torch.full((M, K + 64), float('nan'), dtype=BF, device=dev); X[:, :K] = x.to(dev, BF)
    ops.lora_down(X, A.to(dev, BF), 12, X[:, K:], K)
    close(X[:, K:K + 12], x @ A.T, 1e-2, 1e-2, "lora_down")
    assert X[:, K + 12:].abs().max().item() == 0.0
    dy = rb(torch.randn(M, N, generator=g)); T = X[:, K:K + 16].float().cpu()
    out = torch.zeros(N, r, device=dev)      # in/out: the kernel adds into it
    ops.skinny_tn(dy.to(dev, BF), X[:, K + 4:], r, out, r, 1, 0.25, N)
    close(out, 0.25 * dy.T @ T[:, 4:8], 1e-3, 1e-2, "skinny_tn R=4")
    out16 = torch.zeros(12, K, device=dev)      # in/out: the kernel adds into it
    dT = rb(torch.randn(M, 16, generator=g)); dT[:, 12:] = 0
    ops.skinny_tn(X, dT.to(dev, BF), 12, out16, 1, K, 1.0, K)
    close(out16, dT[:, :12].T @ x, 1e-3, 1e-2, "skinny_tn R=12")
    out16b = torch.zeros(12, K, device=dev)      # in/out: the kernel adds into it
    ops.skinny_tn(X, dT.to(dev, BF), 12, out16b, 1, K, 1.0, K, use_workspace=True)        # two-stage path
    close(out16b, dT[:, :12].T @ x, 1e-3, 1e-2, "skinny_tn R=12 (two-stage)")
    dx = rb(torch.randn(M, K, generator=g)); DX = dx.to(dev, BF).clone()
    ops.lora_up_add(DX, dT.to(dev, BF), A.to(dev, BF), 12, K)
    close(DX, dx + dT[:, :12] @ A, 1e-2, 2e-2, "lora_up_add")
    Bc = torch.randn(3 * N, r, generator=g)
    W = torch.full((3 * N, K + 64), 7.0, dtype=BF, device=dev)      # sentinel: the columns left of the packed slice are asserted below
    ops.lora_pack_b(Bc.to(dev), W[:, K:], K + 64, 3, N, r, 0.25)
    ref = torch.zeros(3 * N, 64)
    for j in range(3):
        ref[j * N:(j + 1) * N, j * r:(j + 1) * r] = 0.25 * Bc[j * N:(j + 1) * N]
    close(W[:, K:], ref, 1e-2, 1e-3, "pack_b"); assert (W[:, :K] == 7).all()
    WT = torch.full((K + 64, 3 * N), 7.0, dtype=BF, device=dev)      # sentinel: the rows above the packed slice
    ops.lora_pack_bt(Bc.to(dev), WT[K:], 3 * N, 3, N, r, 0.25)
    close(WT[K:], ref.T, 1e-2, 1e-3, "pack_bt")


# ------------------------------------------------------------------ weight-gradient GEMM and column reductions (full fine-tune)
@pytest.mark.parametrize("M,P,Q", [(200, 128, 128), (1000, 256, 384), (17776, 1920, 1920), (129, 384, 128), (4500, 1152, 1024), (9001, 640, 1920)])
def test_gemm_nt(dev, M, P, Q):
    from vt355 import ops
    g = torch.Generator().manual_seed(M + P)
    a = rb(torch.randn(M, P + 64, generator=g)); b = rb(torch.randn(M, Q + 8, generator=g))     # strided operands
    ref = a[:, :P].T @ b[:, :Q]
    c = torch.full((P, Q), 3.0, device=dev)      # in/out: accumulate=True adds to the 3.0s; the overwrite call then writes it whole
    ops.gemm_nt(a.to(dev, BF), b.to(dev, BF), c, P=P, Q=Q, alpha=0.5, accumulate=True)
    close(c, 3.0 + 0.5 * ref, 2e-3, 2e-3 * ref.abs().max().item(), "gemm_nt accumulate")
    ops.gemm_nt(a.to(dev, BF), b.to(dev, BF), c, P=P, Q=Q, alpha=1.0, accumulate=False)
    close(c, ref, 2e-3, 2e-3 * ref.abs().max().item(), "gemm_nt overwrite")


@pytest.mark.parametrize("M,P,Q,ru,cu", [(700, 1280, 1152, (80, 72), None), (16384, 3840, 1152, (80, 72), None), (4100, 1152, 1280, None, (80, 72)),
                                         (300, 2560, 128, (80, 72), None), (9000, 640, 1280, (160, 100), (128, 120))])
def test_gemm_nt_unpadded_result(dev, M, P, Q, ru, cu):
    """vt_gemm_nt_bf16_unpad: of every `group` result rows (columns) the first `keep` are stored, packed -- the gradient of OpenSora's
    head-padded projections written straight into the reference-layout buffer; both kernels (weight-sized and small outputs), split
    token ranges (atomics) and the single-range path, accumulate and overwrite; rows outside the result are never touched"""
    from vt355 import ops
    g = torch.Generator().manual_seed(M + P)
    a = rb(torch.randn(M, P + 64, generator=g)); b = rb(torch.randn(M, Q + 8, generator=g))
    full = a[:, :P].T @ b[:, :Q]
    ref = full
    if ru is not None:
        ref = ref.view(P // ru[0], ru[0], -1)[:, :ru[1]].reshape(-1, ref.shape[-1])
    if cu is not None:
        ref = ref.view(ref.shape[0], Q // cu[0], cu[0])[:, :, :cu[1]].reshape(ref.shape[0], -1)
    rows, cols = ref.shape
    big = torch.full((rows + 2, cols + 5), 3.0, device=dev)                   # a guard row above and below, guard columns on the right
    c = big[1:1 + rows, :cols]
    ops.gemm_nt(a.to(dev, BF), b.to(dev, BF), c, P=P, Q=Q, alpha=0.5, accumulate=True, row_unpad=ru, col_unpad=cu)
    close(c, 3.0 + 0.5 * ref, 2e-3, 2e-3 * ref.abs().max().item(), "gemm_nt unpad accumulate")
    ops.gemm_nt(a.to(dev, BF), b.to(dev, BF), c, P=P, Q=Q, alpha=1.0, accumulate=False, row_unpad=ru, col_unpad=cu)
    close(c, ref, 2e-3, 2e-3 * ref.abs().max().item(), "gemm_nt unpad overwrite")
    assert (big[0] == 3.0).all() and (big[-1] == 3.0).all() and (big[:, cols:] == 3.0).all()
    with pytest.raises(Exception):
        ops.gemm_nt(a.to(dev, BF), b.to(dev, BF), c, P=P, Q=Q, row_unpad=(96, 72))          # P is not a multiple of the group


def test_group_colsum(dev):
    from vt355 import ops
    g = torch.Generator().manual_seed(21)
    B, S, St, D = 3, 301, 17, 192
    M = B * S
    x = rb(torch.randn(M, D, generator=g)); y = rb(torch.randn(M, D, generator=g) * 2 + 1)
    mean = y.mean(1); rstd = 1.0 / (y.var(1, unbiased=False) + 1e-5).sqrt()
    o1 = torch.zeros(1, D, device=dev)      # in/out: the kernel adds into it
    ops.group_colsum(x.to(dev, BF), o1)
    close(o1[0], x.sum(0), 1e-4, 1e-3, "colsum")
    o1 = torch.zeros(2 * B, D, device=dev); o2 = torch.zeros(2 * B, D, device=dev)      # in/out: the kernel adds into it
    ops.group_colsum(x.to(dev, BF), o1, y=y.to(dev, BF), out2=o2, mean=mean.to(dev), rstd=rstd.to(dev), S=S, St=St, grouped=True)
    yn = (y - mean[:, None]) * rstd[:, None]
    for b in range(B):
        for seg, rows in ((0, slice(b * S, b * S + St)), (1, slice(b * S + St, (b + 1) * S))):
            close(o1[2 * b + seg], x[rows].sum(0), 1e-4, 2e-3, "group sum")
            close(o2[2 * b + seg], (x[rows] * yn[rows]).sum(0), 1e-4, 3e-3, "group sum of products")


def test_group_colsum_per_sample_groups_whole_rows(dev):
    """adaLN shift / scale gradients of STDiT (one group per sample, no text segment, 4096 rows per sample, 1152 columns): the whole-row kernel
    with blocks that lie inside one sample, sums at out + b * o_bstride + o_segstride"""
    from vt355 import ops
    g = torch.Generator().manual_seed(77)
    B, S, D = 3, 4096, 1152
    M = B * S
    x = rb(torch.randn(M, D, generator=g)); y = rb(torch.randn(M, D, generator=g) * 2 + 1)
    mean = y.mean(1); rstd = 1.0 / (y.var(1, unbiased=False) + 1e-5).sqrt()
    o1 = torch.zeros(B, 6 * D, device=dev); o2 = torch.zeros(B, 6 * D, device=dev)      # in/out: the kernel adds into it; the columns outside the two slices must stay 0
    ops.group_colsum(x.to(dev, BF), o1[:, 3 * D:], y=y.to(dev, BF), out2=o2[:, 4 * D:], mean=mean.to(dev), rstd=rstd.to(dev), D=D, S=S, St=0,
                     grouped=True, o_bstride=6 * D, o_segstride=0)
    yn = (y.double() - mean[:, None].double()) * rstd[:, None].double()
    for b in range(B):
        r1 = x[b * S:(b + 1) * S].double().sum(0); r2 = (x[b * S:(b + 1) * S].double() * yn[b * S:(b + 1) * S]).sum(0)
        close(o1[b, 3 * D:4 * D], r1.float(), 1e-4, 2e-3 * r1.abs().max().item(), "per-sample sum")
        close(o2[b, 4 * D:5 * D], r2.float(), 1e-4, 3e-3 * r2.abs().max().item(), "per-sample sum of products")
    assert o1[:, :3 * D].abs().max().item() == 0 and o1[:, 4 * D:].abs().max().item() == 0


def test_group_colsum_single_sample_group(dev):
    """one sample whose row count is not a multiple of 16 (HunyuanVideo's 10 200 image rows at micro-batch 1): the group IS the matrix -- the
    whole-row kernel with the group's output offset"""
    from vt355 import ops
    g = torch.Generator().manual_seed(78)
    S, D = 4104, 384
    x = rb(torch.randn(S, D, generator=g)); y = rb(torch.randn(S, D, generator=g) * 2 + 1)
    mean = y.mean(1); rstd = 1.0 / (y.var(1, unbiased=False) + 1e-5).sqrt()
    o1 = torch.zeros(1, 3 * D, device=dev); o2 = torch.zeros(1, 3 * D, device=dev)      # in/out: the kernel adds into it; the columns outside the two slices must stay 0
    ops.group_colsum(x.to(dev, BF), o1[:, D:], y=y.to(dev, BF), out2=o2[:, 2 * D:], mean=mean.to(dev), rstd=rstd.to(dev), D=D, S=S, St=0, grouped=True,
                     o_bstride=3 * D, o_segstride=0)
    yn = (y.double() - mean[:, None].double()) * rstd[:, None].double()
    r1 = x.double().sum(0); r2 = (x.double() * yn).sum(0)
    close(o1[0, D:2 * D], r1.float(), 1e-4, 2e-3 * r1.abs().max().item(), "single-group sum")
    close(o2[0, 2 * D:], r2.float(), 1e-4, 3e-3 * r2.abs().max().item(), "single-group sum of products")
    assert o1[0, :D].abs().max().item() == 0 and o1[0, 2 * D:].abs().max().item() == 0


@pytest.mark.parametrize("M,D", [(4096, 320), (5003, 640), (9999, 1024), (4100, 8), (7001, 328), (4500, 324), (16384, 1152), (8200, 4608), (4099, 3456),
                                 (4097, 2056)])
def test_group_colsum_narrow_matrices(dev, M, D):
    """ungrouped column sums of a matrix with a multiple of 8 columns and >= 4096 rows take the whole-row kernel (the UNet's 320 / 640-channel
    bias and GroupNorm-parameter gradients; STDiT's 1152 .. 4608-wide Linear bias gradients, in column slabs), contiguous or strided, with or
    without the product with a normalised second operand; 324 columns fall back to the general kernel -- all equal the fp64 sums, and the sums
    accumulate into the outputs"""
    from vt355 import ops
    g = torch.Generator().manual_seed(M + D)
    x = rb(torch.randn(M, D, generator=g))
    ref = x.double().sum(0)
    o = torch.full((1, D), 3.0, device=dev)      # in/out: the kernel adds into it (3.0 + sums)
    ops.group_colsum(x.to(dev, BF), o)
    close(o[0] - 3.0, ref.float(), 1e-4, 2e-3 * ref.abs().max().item(), "narrow colsum")
    wide = torch.zeros(M, D + 8, dtype=BF, device=dev); wide[:, :D] = x.to(dev, BF)
    o2 = torch.zeros(1, D, device=dev)      # in/out: the kernel adds into it
    ops.group_colsum(wide[:, :D], o2, D=D)
    close(o2[0], ref.float(), 1e-4, 2e-3 * ref.abs().max().item(), "strided colsum")
    y = rb(torch.randn(M, D, generator=g) * 2 + 1)
    mean = y.mean(1); rstd = 1.0 / (y.var(1, unbiased=False) + 1e-5).sqrt()
    for stats in (False, True):
        yn = ((y - mean[:, None]) * rstd[:, None]) if stats else y
        ref2 = (x.double() * yn.double()).sum(0)
        a = torch.zeros(1, D, device=dev); b2 = torch.full((1, D), -1.0, device=dev)      # in/out: the kernel adds into it (b2: -1.0 + sums)
        ops.group_colsum(wide[:, :D], a, y=y.to(dev, BF), out2=b2, mean=mean.to(dev) if stats else None, rstd=rstd.to(dev) if stats else None, D=D)
        close(a[0], ref.float(), 1e-4, 2e-3 * ref.abs().max().item(), "colsum next to the product sums")
        close(b2[0] + 1.0, ref2.float(), 1e-4, 3e-3 * ref2.abs().max().item(), "column sums of x * y")


# ------------------------------------------------------------------ error behaviour of the C-ABI
def test_abi_rejects_bad_arguments(dev):
    """The library validates shapes / alignment on the host and returns a negative code (no launch, no fault): the Python
    binding turns it into VtError.  Mirrors how the reference's own layers fail loudly on shape mismatches."""
    from vt355 import ops
    from vt355._lib import VtError
    a = torch.zeros(64, 128, dtype=BF, device=dev); w = torch.zeros(64, 128, dtype=BF, device=dev)
    out = torch.zeros(64, 64, dtype=BF, device=dev)
    with pytest.raises(VtError, match="vt_gemm_bf16"):              # K not a multiple of the 64-deep K-tile
        ops.gemm(a, w, out, None, K=100)
    with pytest.raises(VtError):                                     # misaligned operand (16-byte rule of the LDS-DMA path)
        ops.gemm(a.view(-1)[4:4 + 63 * 128].view(63, 128), w, out[:63], None)
    with pytest.raises(VtError, match="vt_gemm_nt_bf16"):           # dW tile sizes must be multiples of 128
        ops.gemm_nt(a, w, torch.zeros(100, 128, device=dev), P=100, Q=128)
    with pytest.raises(VtError, match="vt_gemm_set_tile"):
        ops.gemm_set_tile(7)
    with pytest.raises(VtError, match="vt_attn_bwd_set_chain"):      # persistent grid must be a multiple of 8 slots
        ops.attn_bwd_set_chain(0, 12)
    ops.attn_bwd_set_chain(0, 0)
    with pytest.raises(VtError, match="vt_rmsnorm_bf16"):           # rows of 8-element chunks
        ops.rmsnorm(a[:, :60], w[0, :60], out[:, :60])
    with pytest.raises(VtError, match="vt_gated_gelu_bf16"):        # u must hold both halves
        ops.gated_gelu(a, torch.zeros(64, 128, dtype=BF, device=dev))
    with pytest.raises((VtError, TypeError, ValueError)):            # host tensors are refused: there is no CPU path
        ops.gemm(a.cpu(), w.cpu(), out.cpu(), None)


# ------------------------------------------------------------------ frozen T5 text encoder kernels
@pytest.mark.parametrize("M,D", [(5, 64), (452, 4096), (300, 1032)])
def test_rmsnorm(dev, M, D):
    """T5LayerNorm (transformers modeling_t5.T5LayerNorm): x * rsqrt(mean(x^2) + eps) * w, fp32 statistics, strided rows"""
    _rmsnorm_case(dev, M, D)


def _rmsnorm_case(dev, M, D, rows=None):
    """rows: (M, D, generator) -> the bf16-representable input rows, in place of the randn ones (tests/test_conditioning_gpu.py)"""
    from vt355 import ops
    g = torch.Generator().manual_seed(M + D)
    xb = rb(torch.randn(M, D + 8, generator=g) * 3.0); w = rb(1.0 + 0.2 * torch.randn(D, generator=g))
    if rows is not None:
        xb[:, :D] = rows(M, D, g)
    x = xb[:, :D]
    ref = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * w
    X = xb.to(dev, BF)
    y = torch.full((M, D + 16), 9.0, dtype=BF, device=dev)      # sentinel: the pad columns are asserted below
    ops.rmsnorm(X[:, :D], w.to(dev, BF), y[:, :D], 1e-6)
    close(y[:, :D], ref, 1e-2, 1e-2, "rmsnorm"); assert (y[:, D:] == 9).all()


def test_gated_gelu(dev):
    from vt355 import ops
    g = torch.Generator().manual_seed(4)
    M, Fd = 123, 264
    u = rb(torch.randn(M, 2 * Fd + 8, generator=g) * 2.0)
    ref = F.gelu(u[:, :Fd], approximate="tanh") * u[:, Fd:2 * Fd]
    y = poisoned((M, Fd), BF, dev)
    ops.gated_gelu(u.to(dev, BF), y)
    close(y, ref, 1e-2, 1e-2, "gated gelu")


@pytest.mark.parametrize("B,H,S,scale", [(2, 3, 226, 1.0), (1, 2, 77, 0.125), (1, 1, 300, 1.0)])
def test_attn_fwd_bias(dev, B, H, S, scale):
    """softmax(q k^T * scale + bias) v against fp32 torch, bias given transposed [H, key, query] (T5Attention: scale 1, bias =
    relative position table, no mask); ragged S; lse2 = log2 sum exp of the biased scores"""
    from vt355 import ops
    g = torch.Generator().manual_seed(S)
    d = H * 64
    qkv = rb(torch.randn(B, S, 3 * d, generator=g) * (0.35 if scale == 1.0 else 1.0))
    bias = torch.randn(H, S, S, generator=g) * 2.0                       # [h, query, key]
    q, k, v = [qkv[:, :, i * d:(i + 1) * d].view(B, S, H, 64).transpose(1, 2) for i in range(3)]
    s = q @ k.transpose(-1, -2) * scale + bias[None]
    ref = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, S, d)
    lse_ref = torch.logsumexp(s, -1) * 1.4426950408889634
    dqkv = qkv.to(dev, BF)
    o = poisoned((B, S, d), BF, dev); lse = poisoned((B, H, S), torch.float32, dev)
    bias_t = bias.transpose(1, 2).contiguous().to(dev)
    ops.attn_fwd_bias(dqkv[:, :, :d], dqkv[:, :, d:2 * d], dqkv[:, :, 2 * d:], bias_t, o, lse, B, H, S, scale)
    close(o, ref, 2e-2, 2e-2, "attention with bias")
    close(lse, lse_ref, 1e-3, 2e-2, "lse2 with bias")
    with pytest.raises(ValueError):
        ops.attn_fwd_bias(dqkv[:, :, :d], dqkv[:, :, d:2 * d], dqkv[:, :, 2 * d:], bias_t[:, :, :-1].contiguous(), o, lse, B, H, S, scale)


@pytest.mark.parametrize("M,N,K,splits", [(452, 4096, 4096, 0), (452, 512, 10240, 5), (100, 256, 1024, 2), (300, 384, 512, 1)])
def test_gemm_splitk_and_residual_cast(dev, M, N, K, splits):
    """few rows x large weight: K range split over the persistent producer / consumer kernel, fp32 atomics, finishing pass"""
    from vt355 import ops
    from vt355._lib import VtError
    g = torch.Generator().manual_seed(M + N + K)
    a = rb(torch.randn(M, K + 64, generator=g)); w = rb(torch.randn(N, K, generator=g) * 0.05); r = rb(torch.randn(M, N, generator=g))
    ref = a[:, :K] @ w.T
    acc = poisoned((M, N), torch.float32, dev)               # overwritten: the library clears it before the split-K atomics
    ops.gemm_splitk(a.to(dev, BF)[:, :K], w.to(dev, BF), acc, splits)
    close(acc, ref, 2e-3, 2e-3 * ref.abs().max().item(), "split-K accumulate")
    out = poisoned((M, N), BF, dev)
    ops.residual_cast(acc, r.to(dev, BF), out)
    close(out, ref + r, 1e-2, 1e-2 * ref.abs().max().item(), "residual + cast")
    out = poisoned((M, N), BF, dev)
    ops.residual_cast(acc, None, out)
    close(out, ref, 1e-2, 1e-2 * ref.abs().max().item(), "cast")
    with pytest.raises(VtError, match="vt_gemm_splitk_f32"):         # splits must divide K / 64
        ops.gemm_splitk(a.to(dev, BF)[:, :K], w.to(dev, BF), acc, 7 if (K // 64) % 7 else 9)


# ------------------------------------------------------------------ GroupNorm + SiLU, channels-last (first kernel of the VAE / UNet rows)
@pytest.mark.parametrize("N,P,C,G,silu", [(2, 1000, 128, 32, True), (1, 777, 320, 32, True), (3, 64, 512, 32, False),
                                          (1, 13 * 60 * 90, 256, 32, True), (2, 5, 64, 8, True)])
def test_groupnorm_silu_channels_last(dev, N, P, C, G, silu):
    """F.silu(F.group_norm(x, G, gamma, beta, eps)) on [N, C, P] in fp32 vs the channels-last kernel on [N, P, C] bf16
    (10 channels per group at C = 320 like the UNet, 4 at C = 128 like the VAE's first block; strided positions)"""
    from vt355 import ops
    g = torch.Generator().manual_seed(P + C)
    xb = rb(torch.randn(N, P, C + 8, generator=g) * 1.7 + 0.6)
    gamma = rb(1.0 + 0.3 * torch.randn(C, generator=g)); beta = rb(0.2 * torch.randn(C, generator=g))
    x = xb[:, :, :C]
    ref = F.group_norm(x.transpose(1, 2).contiguous(), G, gamma, beta, 1e-6)
    if silu:
        ref = F.silu(ref)
    ref = ref.transpose(1, 2)
    X = xb.to(dev, BF)
    y = torch.full((N, P, C + 16), 5.0, dtype=BF, device=dev)      # sentinel: the pad columns are asserted below
    ops.groupnorm_silu(X[:, :, :C], gamma.to(dev, BF), beta.to(dev, BF), y[:, :, :C], G, 1e-6, silu)
    close(y[:, :, :C], ref, 1e-2, 1.5e-2, "groupnorm+silu"); assert (y[:, :, C:] == 5).all()
    y2 = poisoned((N, P, C), BF, dev)
    ops.groupnorm_silu(X[:, :, :C], None, None, y2, G, 1e-6, False)
    close(y2, F.group_norm(x.transpose(1, 2).contiguous(), G, None, None, 1e-6).transpose(1, 2), 1e-2, 1.5e-2, "groupnorm, no affine")


@pytest.mark.parametrize("N,T,H,W,Cin,Cout", [(1, 3, 5, 7, 64, 64), (2, 4, 9, 10, 128, 256), (1, 1, 16, 12, 64, 132), (1, 5, 20, 33, 256, 128)])
def test_causal_conv3d_channels_last(dev, N, T, H, W, Cin, Cout):
    """implicit-GEMM causal conv3d vs fp32 F.conv3d on the causally padded input (first frame replicated twice in front of t,
    zeros around h / w) -- the padding of the CogVideoX VAE's causal convolutions; tiles that straddle samples, ragged M,
    a single frame, channel-sliced (strided) input and output"""
    from vt355 import ops
    g = torch.Generator().manual_seed(T * H * W + Cin)
    xb = rb(torch.randn(N, T, H, W, Cin + 8, generator=g))
    w = rb(torch.randn(Cout, Cin, 3, 3, 3, generator=g) * (1.0 / (27 * Cin) ** 0.5)); b = rb(torch.randn(Cout, generator=g))
    x = xb[..., :Cin]
    xin = x.permute(0, 4, 1, 2, 3)
    xpad = torch.cat([xin[:, :, :1]] * 2 + [xin], dim=2)
    ref = F.conv3d(xpad, w, b, padding=(0, 1, 1)).permute(0, 2, 3, 4, 1)
    X = xb.to(dev, BF)
    y = torch.full((N, T, H, W, Cout + 4), 3.0, dtype=BF, device=dev)      # sentinel: the pad channels are asserted below
    ops.causal_conv3d(X[..., :Cin], ops.pack_conv3d_weight(w).to(dev, BF), b.to(dev, BF), y[..., :Cout])
    close(y[..., :Cout], ref, 1e-2, 1e-2 * ref.abs().max().item(), "causal conv3d"); assert (y[..., Cout:] == 3).all()
    y2 = poisoned((N, T, H, W, Cout), BF, dev)
    ops.causal_conv3d(X[..., :Cin], ops.pack_conv3d_weight(w).to(dev, BF), None, y2)
    close(y2, ref - b, 1e-2, 1e-2 * ref.abs().max().item(), "causal conv3d, no bias")
    r = rb(torch.randn(N, T, H, W, Cout, generator=g))                      # the ResNet block's skip, added in the epilogue
    y2 = poisoned((N, T, H, W, Cout), BF, dev)
    ops.causal_conv3d(X[..., :Cin], ops.pack_conv3d_weight(w).to(dev, BF), b.to(dev, BF), y2, residual=r.to(dev, BF))
    close(y2, ref + r, 1e-2, 1e-2 * (ref + r).abs().max().item(), "causal conv3d + residual")


@pytest.mark.parametrize("N,T,H,W,Cin,Cout", [(1, 2, 6, 8, 64, 64), (2, 3, 10, 14, 128, 128), (1, 1, 32, 20, 256, 64)])
def test_downsample_conv2d_channels_last(dev, N, T, H, W, Cin, Cout):
    """the VAE's spatial downsample (DownSample3D.forward, cp_enc_dec.py:660-666): F.pad (0,1,0,1) then Conv2d(3, stride 2) per frame"""
    from vt355 import ops
    g = torch.Generator().manual_seed(H * W + Cin)
    x = rb(torch.randn(N, T, H, W, Cin, generator=g))
    w = rb(torch.randn(Cout, Cin, 3, 3, generator=g) * (1.0 / (9 * Cin) ** 0.5)); b = rb(torch.randn(Cout, generator=g))
    xin = x.permute(0, 1, 4, 2, 3).reshape(N * T, Cin, H, W)
    ref = F.conv2d(F.pad(xin, (0, 1, 0, 1)), w, b, stride=2).reshape(N, T, Cout, H // 2, W // 2).permute(0, 1, 3, 4, 2)
    y = poisoned((N, T, H // 2, W // 2, Cout), BF, dev)
    ops.downsample_conv2d(x.to(dev, BF), ops.pack_conv_weight(w).to(dev, BF), b.to(dev, BF), y)
    close(y, ref, 1e-2, 1e-2 * ref.abs().max().item(), "downsample conv2d")


@pytest.mark.parametrize("T", [2, 7, 8, 16, 48])
def test_temporal_pool_all_pairs(dev, T):
    """DownSample3D's plain avg_pool1d branch (cp_enc_dec.py:658-667; diffusers' rule for an even frame count): pairs (0,1),(2,3).."""
    from vt355 import ops
    g = torch.Generator().manual_seed(T)
    N, H, W, C = 2, 3, 5, 64
    x = rb(torch.randn(N, T, H, W, C, generator=g))
    xt = x.permute(0, 2, 3, 4, 1).reshape(N * H * W, C, T)
    ref = F.avg_pool1d(xt, kernel_size=2, stride=2)
    ref = ref.reshape(N, H, W, C, T // 2).permute(0, 4, 1, 2, 3)
    y = poisoned((N, T // 2, H, W, C), BF, dev)
    ops.temporal_pool(x.to(dev, BF), y, keep_first=False)
    close(y, ref, 1e-2, 1e-2, "temporal pool (all pairs)")


@pytest.mark.parametrize("T", [1, 2, 5, 8, 49])
def test_temporal_pool(dev, T):
    """DownSample3D's compress_time branch (cp_enc_dec.py:640-657): first frame kept, avg_pool1d(2, 2) over the rest"""
    from vt355 import ops
    g = torch.Generator().manual_seed(T)
    N, H, W, C = 2, 3, 5, 64
    x = rb(torch.randn(N, T, H, W, C, generator=g))
    if T > 1:
        xt = x.permute(0, 2, 3, 4, 1).reshape(N * H * W, C, T)
        rest = F.avg_pool1d(xt[..., 1:], kernel_size=2, stride=2) if T > 2 else xt[..., 1:1]
        ref = torch.cat([xt[..., :1], rest], dim=-1)
        To = ref.shape[-1]
        ref = ref.reshape(N, H, W, C, To).permute(0, 4, 1, 2, 3)
    else:
        ref, To = x, 1
    assert To == 1 + (T - 1) // 2
    y = poisoned((N, To, H, W, C), BF, dev)
    ops.temporal_pool(x.to(dev, BF), y)
    close(y, ref, 1e-2, 1e-2, "temporal pool")


@pytest.mark.parametrize("N,T,H,W,Cin,Cout", [(1, 3, 6, 9, 3, 64), (2, 5, 12, 10, 3, 128), (1, 1, 8, 8, 8, 132)])
def test_causal_conv3d_rgb_input(dev, N, T, H, W, Cin, Cout):
    """the encoder's first convolution: 8 channels per position (Cin of them used), 8 taps per K-tile, vs fp32 F.conv3d"""
    from vt355 import ops
    g = torch.Generator().manual_seed(H * W + Cout)
    x = rb(torch.randn(N, T, H, W, Cin, generator=g))
    w = rb(torch.randn(Cout, Cin, 3, 3, 3, generator=g) * (1.0 / (27 * Cin) ** 0.5)); b = rb(torch.randn(Cout, generator=g))
    xin = x.permute(0, 4, 1, 2, 3)
    ref = F.conv3d(torch.cat([xin[:, :, :1]] * 2 + [xin], dim=2), w, b, padding=(0, 1, 1)).permute(0, 2, 3, 4, 1)
    x8 = torch.zeros(N, T, H, W, 8, dtype=BF, device=dev)
    x8[..., :Cin] = x.to(dev, BF)
    y = poisoned((N, T, H, W, Cout), BF, dev)
    ops.causal_conv3d_in8(x8, ops.pack_conv_in8_weight(w).to(dev, BF), b.to(dev, BF), y)
    close(y, ref, 1e-2, 1e-2 * ref.abs().max().item(), "first conv (8-channel input)")
