"""GPU parity on ill-conditioned inputs (tests/conditioning_ref.py; what they break and reach is asserted on the CPU in
tests/test_conditioning_cpu.py):
  * GroupNorm (+ SiLU) forward, its statistics planes and its backward where the mean dominates the spread -- csrc/groupnorm.hip sums about
    a per-channel pivot; a one-pass `E[x^2] - mean^2` in fp32 returns rounding noise for the variance here;
  * the head_dim-128 and the generic-head-dim flash attention where the running maximum moves late in the key loop, in every tile
    position, and where a masked key would move it if the mask were applied too late;
  * the LayerNorm family (two-pass in registers today) on rows that a one-pass rewrite would get wrong.
Every reference is fp64 on the same bf16-rounded inputs; the bars are those of the kernels' older tests."""
import pytest
import torch

import conditioning_ref as CR
from parity import close, poisoned, untouched

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------ GroupNorm
def _groupnorm_case(dev, name, P, C, G, pad=0, accumulate=False):
    """forward into a poisoned [N, P, C + pad] buffer from a strided x, the statistics planes of the workspace, backward (dx into a
    poisoned strided buffer, or added to a base with accumulate)"""
    from vt355 import ops
    c = CR.gn_case(name, P, C, G); ref = CR.gn_reference(name, P, C, G)
    x, eps, silu = c["x"], c["eps"], c["silu"]
    N, cpg = x.shape[0], C // G
    X = torch.zeros(N, P, C + pad, dtype=BF, device=dev); X[:, :, :C] = x.to(dev, BF)
    xd = X[:, :, :C]
    ga, be = c["gamma"].to(dev, BF), c["beta"].to(dev, BF)
    Y = poisoned((N, P, C + pad), BF, dev)
    ws = ops.groupnorm_fwd(xd, ga, be, Y[:, :, :C], G, eps, silu)
    planes = ws.view(N, 4, C)
    mean_c, rstd_c = planes[:, 0], planes[:, 1]                      # per channel, equal within a group
    mean = mean_c.view(N, G, cpg); rstd = rstd_c.view(N, G, cpg)
    assert bool((mean == mean[:, :, :1]).all()) and bool((rstd == rstd[:, :, :1]).all()), "statistics differ within a group"
    rel = ((rstd[:, :, 0].double().cpu() / ref["rstd"]) - 1).abs().max().item()
    print(f"[groupnorm {name} N={N} P={P} C={C} G={G}] rstd: largest relative error {rel:.3g}")
    close(rstd[:, :, 0], ref["rstd"], CR.GN_STAT_RTOL, 0.0, "groupnorm rstd")
    close(mean[:, :, 0], ref["mean"], CR.GN_STAT_RTOL, CR.GN_STAT_ATOL_MEAN, "groupnorm mean")
    close(Y[:, :, :C], ref["y"], 1e-2, 1.5e-2, "groupnorm+silu")
    untouched(Y, (slice(None), slice(None), slice(0, C)), "groupnorm pad columns")
    dyd = torch.zeros(N, P, C + pad, dtype=BF, device=dev); dyd[:, :, :C] = c["dy"].to(dev, BF)
    dga = torch.zeros(C, device=dev); dbe = torch.zeros(C, device=dev)
    gmax = ref["dx"].abs().max().item()
    if accumulate:
        base = CR.rb(torch.randn(N, P, C, generator=torch.Generator().manual_seed(3)))
        DX = torch.zeros(N, P, C + pad, dtype=BF, device=dev); DX[:, :, :C] = base.to(dev, BF)
        ops.groupnorm_bwd(dyd[:, :, :C], xd, ga, ws, DX[:, :, :C], dga, dbe, G, silu, accumulate=True)
        close(DX[:, :, :C], ref["dx"] + base.double(), 3e-2, 3e-2 * gmax, "groupnorm dx (accumulate)")
        assert bool((DX[:, :, C:] == 0).all())
    else:
        DX = poisoned((N, P, C + pad), BF, dev)
        ops.groupnorm_bwd(dyd[:, :, :C], xd, ga, ws, DX[:, :, :C], dga, dbe, G, silu)
        close(DX[:, :, :C], ref["dx"], 3e-2, 2e-2 * gmax, "groupnorm dx")
        untouched(DX, (slice(None), slice(None), slice(0, C)), "groupnorm dx pad columns")
    close(dga, ref["dgamma"], 2e-2, 2e-2 * ref["dgamma"].abs().max().item(), "groupnorm dgamma")
    close(dbe, ref["dbeta"], 2e-2, 2e-2 * ref["dbeta"].abs().max().item(), "groupnorm dbeta")


@pytest.mark.parametrize("P,C,G", CR.GN_SHAPES)
@pytest.mark.parametrize("name", CR.GN_CASES)
def test_groupnorm_ill_conditioned(dev, name, P, C, G):
    """8, 10 (an 8-channel chunk straddles two groups) and 80 channels per group (two channel passes); contiguous rows"""
    _groupnorm_case(dev, name, P, C, G)


@pytest.mark.parametrize("name", ["plateau", "two_samples"])
def test_groupnorm_ill_conditioned_strided(dev, name):
    """rows C + 8 apart: the pad columns of y and dx keep their poison, those of x and dy are never read into a statistic"""
    _groupnorm_case(dev, name, *CR.GN_SHAPES[1], pad=8)


def test_groupnorm_ill_conditioned_accumulate(dev):
    _groupnorm_case(dev, "plateau_small", *CR.GN_SHAPES[0], pad=8, accumulate=True)


# ------------------------------------------------------------------------------------------------ attention, head_dim 128 long-sequence kernels
@pytest.mark.parametrize("B,S,H,lens", [(1, 333, 2, None), (1, 333, 2, (300,))], ids=["full", "kv300"])
@pytest.mark.parametrize("name", CR.SOFTMAX_CASES)
def test_attn128_late_maximum(dev, name, B, S, H, lens):
    """the rescale branch after tile 0, a stale reference, and (kv300, late_spike) a masked x 12 key that must move nothing and get
    exactly zero dK / dV -- the assertions are test_attn128_matches_dense_attention's"""
    from test_hunyuan_gpu import attn128_case
    g = torch.randn(B, S, H * 128, generator=torch.Generator().manual_seed(S)).to(BF)
    attn128_case(dev, CR.softmax_qkv(name, B, S, H), g, H, lens)


def test_attn128_masked_giant_key_moves_nothing(dev):
    """key 301 x 150 behind kv_len = 300, inside the last key tile the kernel loads: a reference moved by it would underflow every valid
    key's weight (the x 12 key 330 of late_spike is never loaded at kv_len = 300, and a reference too high by 70 log2 units would still
    be divided out exactly)"""
    from test_hunyuan_gpu import attn128_case
    B, S, H = 1, 333, 2
    g = torch.randn(B, S, H * 128, generator=torch.Generator().manual_seed(S + 2)).to(BF)
    attn128_case(dev, CR.softmax_qkv("masked_giant", B, S, H), g, H, (300,))


@pytest.mark.parametrize("hd", [72, 128])
def test_attn_gen_masked_giant_key_moves_nothing(dev, hd):
    from test_unet_kernels_gpu import _gen_case
    _gen_case(dev, 1, 2, 333, 333, hd, 80 if hd == 72 else 128, kv_len=[300], bf16_out=True, shape_keys=lambda k: CR.scale_keys(k, "masked_giant"))


@pytest.mark.parametrize("name", CR.SOFTMAX_CASES)
def test_attn128_late_maximum_two_samples(dev, name):
    from test_hunyuan_gpu import attn128_case
    B, S, H = 2, 333, 2
    g = torch.randn(B, S, H * 128, generator=torch.Generator().manual_seed(S + 1)).to(BF)
    attn128_case(dev, CR.softmax_qkv(name, B, S, H), g, H, (333, 137))


# ------------------------------------------------------------------------------------------------ attention, generic head dim
@pytest.mark.parametrize("hd", [72, 128])
@pytest.mark.parametrize("name", CR.SOFTMAX_CASES)
def test_attn_gen_late_maximum(dev, name, hd):
    """vt_attn_gen's online softmax per key tile: 333 queries x 333 keys, then with per-sample valid lengths (the late spike masked in
    sample 0) and bf16 dK / dV, whose padded rows must come back exactly 0"""
    from test_unet_kernels_gpu import _gen_case
    hs = 80 if hd == 72 else 128
    shape = lambda k: CR.scale_keys(k, name)
    _gen_case(dev, 1, 2, 333, 333, hd, hs, shape_keys=shape)
    _gen_case(dev, 2, 2, 333, 333, hd, hs, kv_len=[300, 137], bf16_out=True, shape_keys=shape)


@pytest.mark.parametrize("name", CR.SOFTMAX_CASES)
def test_attn_gen_late_maximum_query_split(dev, name):
    """many queries, few keys: the query range is split over workgroups, every one of them walks the same two key tiles"""
    from test_unet_kernels_gpu import _gen_case
    _gen_case(dev, 2, 2, 4096, 120, 72, 80, kv_len=[37, 120], shape_keys=lambda k: CR.scale_keys(k, name))


# ------------------------------------------------------------------------------------------------ LayerNorm family (guards)
@pytest.mark.parametrize("D", [128, 1920, 3072])
@pytest.mark.parametrize("kind", CR.LN_ROWS)
def test_ln_modulate_ill_conditioned_rows(dev, kind, D):
    """1, 4 and 8 chunks of 8 elements per lane (the three template branches); forward, mean / rstd against fp64 at 1e-4, backward"""
    from test_kernels_gpu import _ln_modulate_case
    _ln_modulate_case(dev, D, rows=lambda M, D_, g: CR.ln_rows(kind, M, D_, g))


@pytest.mark.parametrize("kind", CR.LN_ROWS)
def test_ln_modulate_fwd_fp8_ill_conditioned_rows(dev, kind):
    from test_hunyuan_mxfp8_gpu import ln_modulate_fwd_fp8_case
    ln_modulate_fwd_fp8_case(dev, rows=lambda M, D, g: CR.ln_rows(kind, M, D, g))


@pytest.mark.parametrize("kind", CR.LN_ROWS)
def test_qk_layernorm_ill_conditioned_rows(dev, kind):
    from test_kernels_gpu import _qk_layernorm_case
    _qk_layernorm_case(dev, rows=lambda M, D, g: CR.ln_rows(kind, M, D, g))


@pytest.mark.parametrize("kind", CR.LN_ROWS)
def test_qk_rmsnorm_rope128_ill_conditioned_rows(dev, kind):
    from test_hunyuan_gpu import qk_rmsnorm_rope128_case
    qk_rmsnorm_rope128_case(dev, 27, 37, 0, True, rows=lambda M, D, g: CR.ln_rows(kind, M, D, g))


@pytest.mark.parametrize("kind", CR.LN_ROWS)
def test_rmsnorm_ill_conditioned_rows(dev, kind):
    from test_kernels_gpu import _rmsnorm_case
    _rmsnorm_case(dev, 300, 1032, rows=lambda M, D, g: CR.ln_rows(kind, M, D, g))
