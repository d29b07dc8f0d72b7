"""vt_attn_fwd_hd64 (plain, pre-scaled, 16x16x32 tiles), vt_attn_fwd_bias_hd64 and vt_attn_bwd_hd64 against fp64 dense attention
(tests/attn64_ref.py) where tests/test_kernels_gpu.py does not go: sizes below one key tile and one past every tile boundary, separate
strided buffers with pad columns, inputs whose row maximum arrives late (the forward's lazy reference rescales, and leaves stale references),
and the smallest shapes at which the backward really forms a dQ hand-off chain.

The bars are those of test_attn_fwd / test_attn_bwd: o 2e-2 / 1e-2, lse2 ln2 1e-4 / 2e-3, gradients 3e-2 / 1e-2 max|ref|.
The backward is fed o (bf16) and lse2 (fp32) of the fp64 reference, never the kernel's own forward: a wrong forward and a wrong backward
stay apart.  Every output is a poisoned buffer; whatever lies outside a kernel's contract region must still hold the poison afterwards."""
import math

import pytest
import torch

import attn64_ref as R
from conditioning_ref import SOFTMAX_CASES
from parity import close, poisoned, untouched

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
LN2 = math.log(2.0)
VARIANTS = ("plain", "prescaled", "tiles16")


def _padded(t, pad, slack, dev):
    """t [B, S, D] as a view into a buffer of [B, S + slack, D + pad] whose pad columns and slack rows hold NaN: an input the kernel must
    never let into a result (rows past S of a ragged tile are out of range of its buffer descriptors, or masked)"""
    B, S, D = t.shape
    buf = poisoned((B, S + slack, D + pad), BF, dev)
    buf[:, :S, :D] = t.to(dev, BF)
    return buf[:, :S, :D]


# ------------------------------------------------------------------ forward
def _fwd_fused(dev, name, B, S, H, variant):
    """the fused [B, S, 3 H 64] view test_attn_fwd uses, contiguous outputs"""
    from vt355 import ops
    pre = variant != "plain"
    qkv, _ = R.qkv_case(name, B, S, H, pre)
    ref = R.reference(name, B, S, H, pre)
    D = H * 64
    d = qkv.to(dev, BF).view(B, S, 3 * D)
    o = poisoned((B, S, D), BF, dev)
    lse2 = poisoned((B, H, S), torch.float32, dev)
    ops.attn_fwd(d[:, :, :D], d[:, :, D:2 * D], d[:, :, 2 * D:], o, lse2, B, H, S, q_prescaled=pre, tiles16=variant == "tiles16")
    what = f"{name} B{B} S{S} H{H} {variant}"
    close(o, ref["o"], 2e-2, 1e-2, "o " + what)
    close(lse2 * LN2, ref["lse2"] * LN2, 1e-4, 2e-3, "lse " + what)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("S", R.FWD_EDGE_S)
def test_fwd_tile_edges(dev, S, variant):
    """128 query rows per workgroup, 32 per wave, 64-key tiles: one key, less than a tile, and one past 64 / 128 / 192 / 256"""
    _fwd_fused(dev, "randn", 2, S, 3, variant)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B,H,S", R.FWD_LATE)
@pytest.mark.parametrize("name", SOFTMAX_CASES)
def test_fwd_late_maximum(dev, name, B, H, S, variant):
    """every wave takes the rescale branch after tile 0, in every tile position over the three families, and hundreds of rows end with a
    reference up to 8 below their maximum (tests/test_attn64_cpu.py); the plain kernel moves its maximum at every tile"""
    _fwd_fused(dev, name, B, S, H, variant)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("S", R.FWD_SPIKE_S)
def test_fwd_spike_in_a_ragged_tile(dev, S, variant):
    """S = 65, 129: the last tile holds one key and 63 masked scores, the x 12 key ends the full tile in front of it (at 65 that is tile 0: the
    reference never moves again).  S = 67, 131: the x 12 key leads a three-key ragged tile, which rescales against 61 masked scores."""
    _fwd_fused(dev, "late_spike", 2, S, 3, variant)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("S", [31, 67])
def test_fwd_all_scores_far_below_zero(dev, S, variant):
    """every real score near -185 log2 units: the zero score of a key past S (before its mask) towers over them.  Tile 0 of S = 31 and tile 1
    of S = 67 hold 33 / 61 such keys; they must move neither the maximum nor the reference"""
    _fwd_fused(dev, "all_low", 2, S, 3, variant)


@pytest.mark.parametrize("variant", VARIANTS)
def test_fwd_reference_never_moves_down_after_tile_0(dev, variant):
    """early_giant: rows that end tile 0 with a reference 130 .. 200 above everything later sit in waves that rescale at tile 1 for another
    row's sake; their own step must be max(rise, 0) = 0 (tests/test_attn64_cpu.py shows such waves exist)"""
    _fwd_fused(dev, "early_giant", 2, 129, 3, variant)


@pytest.mark.parametrize("variant", VARIANTS)
def test_fwd_separate_strided_buffers(dev, variant):
    """q, k, v, o in four buffers of their own: row strides H 64 + 8 | + 64 | + 16 | + 4, batch strides with slack rows, o 8-byte aligned only
    (it starts at column 4 of its buffer).  Pad columns and slack rows of o keep their poison; lse2 is written whole."""
    from vt355 import ops
    B, S, H = 2, 129, 5
    D = H * 64
    pre = variant != "plain"
    qkv, _ = R.qkv_case("randn", B, S, H, pre)
    ref = R.reference("randn", B, S, H, pre)
    x = qkv.view(B, S, 3, D)

    q, k, v = _padded(x[:, :, 0], 8, 1, dev), _padded(x[:, :, 1], 64, 2, dev), _padded(x[:, :, 2], 16, 3, dev)
    obuf = poisoned((B, S + 2, D + 4), BF, dev)
    o = obuf[:, :S, 4:]
    assert (q.stride(1), k.stride(1), v.stride(1), o.stride(1)) == (D + 8, D + 64, D + 16, D + 4)
    assert o.data_ptr() % 16 == 8 and o.stride(0) == (S + 2) * (D + 4)
    lse2 = poisoned((B, H, S), torch.float32, dev)
    ops.attn_fwd(q, k, v, o, lse2, B, H, S, q_prescaled=pre, tiles16=variant == "tiles16")
    close(o, ref["o"], 2e-2, 1e-2, "o, strided " + variant)
    close(lse2 * LN2, ref["lse2"] * LN2, 1e-4, 2e-3, "lse, strided " + variant)
    untouched(obuf, (slice(None), slice(0, S), slice(4, None)), "o pad columns / slack rows " + variant)


def _bias_reference(qkv64, bias, B, S, H, scale):
    q, k, v = [qkv64[:, :, i].permute(0, 2, 1, 3) for i in range(3)]                 # [B,H,S,64]
    s = q @ k.transpose(-1, -2) * scale + bias.double()[None]
    o = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B, S, H * 64)
    return o, torch.logsumexp(s, -1)


@pytest.mark.parametrize("S,late", [(1, False), (63, False), (65, False), (226, False), (226, True)],
                         ids=["S1", "S63", "S65", "S226", "S226_late_bias"])
def test_fwd_bias_edges_and_a_late_maximum_in_the_bias(dev, S, late):
    """vt_attn_fwd_bias_hd64 (T5: softmax(q k^T scale + bias) v, bias transposed [H, key, query]).  late: the bias adds + 40 to key S - 2 for
    every third query -- the maximum arrives in the last tile and is carried by the bias, not by K"""
    from vt355 import ops
    B, H, scale = 2, 3, 0.125
    D = H * 64
    qkv, ref64 = R.qkv_case("randn", B, S, H, False)
    bias = 2.0 * torch.randn(H, S, S, generator=torch.Generator().manual_seed(S))        # [h, query, key]
    if late:
        bias[:, ::3, S - 2] += 40.0
    o_ref, lse_ref = _bias_reference(ref64, bias, B, S, H, scale)
    d = qkv.to(dev, BF).view(B, S, 3 * D)
    o = poisoned((B, S, D), BF, dev); lse2 = poisoned((B, H, S), torch.float32, dev)
    ops.attn_fwd_bias(d[:, :, :D], d[:, :, D:2 * D], d[:, :, 2 * D:], bias.transpose(1, 2).contiguous().to(dev), o, lse2, B, H, S, scale)
    close(o, o_ref, 2e-2, 1e-2, "o with bias")
    close(lse2 * LN2, lse_ref, 1e-4, 2e-3, "lse with bias")


# ------------------------------------------------------------------ backward
def _bwd_inputs(dev, name, B, S, H, pre):
    qkv, _ = R.qkv_case(name, B, S, H, pre)
    ref = R.reference(name, B, S, H, pre)
    D = H * 64
    x = qkv.view(B, S, 3, D)
    return x, ref["o"].float(), R.grad_out(B, S, H), ref["lse2"].float().to(dev), ref, D


def _check_grads(dq, dk, dv, ref, B, S, H, what):
    g = ref["dqkv"]
    scale = g.abs().max().item()
    for got, r, n in ((dq, g[:, :, 0], "dq"), (dk, g[:, :, 1], "dk"), (dv, g[:, :, 2], "dv")):
        close(got.reshape(B, S, H, 64), r, 3e-2, 1e-2 * scale, f"{n} {what}")


def _bwd_fused(dev, name, B, S, H, pre, ws=None):
    """fused qkv view, contiguous o / dO / dq / dk / dv; o and lse2 from the fp64 reference; dq zeroed by the caller as the header requires"""
    from vt355 import ops
    x, o_ref, do, lse2, ref, D = _bwd_inputs(dev, name, B, S, H, pre)
    d = x.to(dev, BF).view(B, S, 3 * D)
    dq = torch.zeros(B, S, D, dtype=torch.float32, device=dev)
    dk = poisoned((B, S, D), BF, dev); dv = poisoned((B, S, D), BF, dev)
    delta = poisoned((B * H * S,), torch.float32, dev)
    ops.attn_bwd(d[:, :, :D], d[:, :, D:2 * D], d[:, :, 2 * D:], o_ref.to(dev, BF), do.to(dev, BF), lse2, delta, dq, dk, dv, B, H, S,
                 q_prescaled=pre, chain_ws=ws)
    return dq, dk, dv, ref


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("S", R.BWD_EDGE_S)
def test_bwd_tile_edges_atomics(dev, S, pre):
    """256 keys per workgroup, 32 per wave, 64-query steps, the RAGGED instantiation whenever S is no multiple of 256; no workspace, so every
    key block adds its dQ atomically"""
    from vt355 import ops
    B, H = 2, 2
    assert ops.attn_bwd_chain_plan(B, H, S, have_ws=False)[0] == 1
    dq, dk, dv, ref = _bwd_fused(dev, "randn", B, S, H, pre)
    _check_grads(dq, dk, dv, ref, B, S, H, f"S{S} pre={pre}")


@pytest.mark.parametrize("B,H,S", R.BWD_LATE)
@pytest.mark.parametrize("name", SOFTMAX_CASES)
def test_bwd_late_maximum(dev, name, B, H, S):
    """P rebuilt from lse2 on the inputs whose scores span tens of log2 units inside a row"""
    dq, dk, dv, ref = _bwd_fused(dev, name, B, S, H, True)
    _check_grads(dq, dk, dv, ref, B, S, H, f"{name} S{S}")


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
def test_bwd_separate_strided_buffers(dev, pre):
    """all eight tensors in buffers of their own with distinct row strides; dk row stride H 64 + 4 with the pad behind the row, dv the same with
    the pad in front (8-byte aligned only), dq row stride H 64 + 8.  The pads of dk / dv keep their poison, those of dq are still 0."""
    from vt355 import ops
    B, S, H = 2, 257, 3
    x, o_ref, do, lse2, ref, D = _bwd_inputs(dev, "randn", B, S, H, pre)

    q, k, v = _padded(x[:, :, 0], 8, 1, dev), _padded(x[:, :, 1], 64, 2, dev), _padded(x[:, :, 2], 16, 0, dev)
    o, dO = _padded(o_ref, 24, 3, dev), _padded(do, 40, 1, dev)
    dqbuf = torch.zeros(B, S + 1, D + 8, dtype=torch.float32, device=dev)
    dkbuf = poisoned((B, S + 1, D + 4), BF, dev); dvbuf = poisoned((B, S + 2, D + 4), BF, dev)
    dq, dk, dv = dqbuf[:, :S, :D], dkbuf[:, :S, :D], dvbuf[:, :S, 4:]
    strides = [t.stride(1) for t in (q, k, v, o, dO, dq, dk, dv)]
    assert strides == [D + 8, D + 64, D + 16, D + 24, D + 40, D + 8, D + 4, D + 4] and dv.data_ptr() % 16 == 8
    delta = poisoned((B * H * S,), torch.float32, dev)
    ops.attn_bwd(q, k, v, o, dO, lse2, delta, dq, dk, dv, B, H, S, q_prescaled=pre, chain_ws=None)
    _check_grads(dq, dk, dv, ref, B, S, H, f"strided pre={pre}")
    untouched(dkbuf, (slice(None), slice(0, S), slice(0, D)), "dk pad columns / slack rows")
    untouched(dvbuf, (slice(None), slice(0, S), slice(4, None)), "dv pad columns / slack rows")
    assert bool((dqbuf[:, :, D:] == 0).all()) and bool((dqbuf[:, S:] == 0).all()), "dq pad columns / slack rows were added to"


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("name", R.CHAIN_FAMILIES)
@pytest.mark.parametrize("case", list(R.CHAIN_CASES))
def test_bwd_small_chains(dev, case, name, pre):
    """the smallest launches in which a dQ tile is really handed on (attn64_ref.CHAIN_CASES): the plan is asserted through
    vt_attn_bwd_chain_plan before the launch, the per-launch error word is 0 after it and the sticky time-out count has not moved"""
    from vt355 import ops
    B, H, S, L, slots, _ = R.CHAIN_CASES[case]
    ops.attn_bwd_set_chain(L, slots)
    try:
        assert ops.attn_bwd_chain_plan(B, H, S, have_ws=True) == R.chain_plan_expected(case)
        assert ops.attn_bwd_chain_plan(B, H, S, have_ws=False)[0] == 1
        ws = ops.attn_bwd_chain_workspace(B, H, S, dev)
        assert ws is not None
        sticky = ops.attn_bwd_chain_errors()
        dq, dk, dv, ref = _bwd_fused(dev, name, B, S, H, pre, ws=ws)
        assert ops.attn_bwd_chain_error(ws) == 0
        assert ops.attn_bwd_chain_errors() == sticky
    finally:
        ops.attn_bwd_set_chain(0, 0)
    _check_grads(dq, dk, dv, ref, B, S, H, f"{case} {name} pre={pre}")
