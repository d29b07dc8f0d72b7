"""The memory-bound glue kernels (csrc/elementwise.hip, the GEGLU / row-map / loss / q-sample sections of csrc/unet_ops.hip, the
gated-GELU and residual-cast kernels of csrc/t5.hip) against the fp64 restatements of tests/glue_ref.py: past one sweep of their capped
grids (glue_ref.SWEEPS), on column slices of wider buffers with leading dimensions that differ from operand to operand, with the
aliasing the models rely on, in every variant that ships, and at the smallest sizes.

Bars come from rounding, never from the code under test:
  MOVE   pure data movement: bit-equal.
  ONCE   one fp32 operation and one bf16 store: bit-equal to the fp64 result rounded once (tests/test_glue_ref_cpu.py shows on 2^22
         draws that the fp32 intermediate adds no second rounding for a sum; for gate_mul's bf16 x fp32 product it can, so gate_mul
         is compared with the fp32 restatement of the same single operation).
  ULP    a short fp32 expression and one bf16 store: |got - ref| <= 2^-8 * sum|terms| -- one bf16 ulp on the magnitude of the terms,
         so cancellation is not charged to the kernel; covers fp32 rounding inside the expression and FMA contraction either way.
  FUNC   transcendental kernels: 2^-8 * |ref| + 2 * E, E = max |fp32 restatement - fp64 restatement| of the same formula on rows
         sampled from the same inputs, evaluated on the CPU (printed by the test; the figure seen is in each docstring).
Inputs live inside poisoned buffers: a kernel that indexed with a width in place of a leading dimension reads the NaN poison, and
whatever it writes outside its contract region is caught by `untouched`."""
import math

import pytest
import torch

import glue_ref as R
from parity import is_poison, poisoned, untouched

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
ULP = 2.0 ** -8


# ------------------------------------------------------------------ helpers
def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _slab(rows, cols, ld, off, dtype, dev):
    """(poisoned [rows, ld] buffer, its column slice [:, off:off+cols])"""
    buf = poisoned((rows, ld), dtype, dev)
    return buf, buf[:, off:off + cols]


def _rand_in(rows, cols, ld, off, dev, gen, scale=1.0, dtype=BF):
    """randn * scale in a column slice of a poisoned buffer"""
    _, v = _slab(rows, cols, ld, off, dtype, dev)
    v.copy_((torch.randn(rows, cols, device=dev, generator=gen) * scale).to(dtype))
    return v


def _cols(off, n):
    return (slice(None), slice(off, off + n))


def _within(got, ref, bound, what):
    """|got - ref| <= bound elementwise, on the device; NaN / Inf / poison in got are out of bounds"""
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} against {tuple(ref.shape)}"
    assert bool(torch.isfinite(ref).all()), f"{what}: non-finite reference (a bug of the test)"
    err = (got.double() - ref).abs()
    bound = bound if isinstance(bound, torch.Tensor) else torch.full_like(ref, bound)
    ok = err <= bound
    if not bool(ok.all()):
        ratio = torch.where(ok, torch.zeros_like(err), torch.nan_to_num(err / bound.clamp_min(1e-300), nan=math.inf, posinf=math.inf))
        at = int(ratio.flatten().argmax())
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} past the bound, worst at flat {at}: got {got.flatten()[at].item():.8g} "
                             f"ref {ref.flatten()[at].item():.8g} bound {bound.flatten()[at].item():.3g}")


def _bits_equal(got, want, what):
    a, b = got.contiguous(), want.contiguous()
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype} {tuple(a.shape)} against {b.dtype} {tuple(b.shape)}"
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    ne = a.view(it) != b.view(it)
    assert not bool(ne.any()), f"{what}: {int(ne.sum())} of {ne.numel()} elements differ in their bits (first at flat {int(ne.flatten().int().argmax())})"


def _once(x64):
    return R.round_once_bf16(x64).to(BF)


def _func_error(f, inputs, rows=192):
    """E of the FUNC bar: max |f(fp32 inputs) - f(fp64 inputs)| on the CPU over `rows` rows spread over the inputs (first to last)"""
    M = inputs[0].shape[0]
    idx = torch.linspace(0, M - 1, min(rows, M), device=inputs[0].device).long().unique()
    cpu = [t[idx].float().cpu() for t in inputs]
    return (f(*cpu).double() - f(*[t.double() for t in cpu])).abs().max().item()


WIDE = (R.sweep("vt_geglu_fwd")["shape"]["M"], R.sweep("vt_geglu_fwd")["shape"]["F"])
ROW_CASES = [pytest.param(*WIDE, id="wrap"), pytest.param(1, 2056, id="M1"), pytest.param(37, 8, id="F8")]


# ------------------------------------------------------------------ GEGLU, gated GELU
@pytest.mark.parametrize("M,F", ROW_CASES)
def test_geglu_forward_backward(dev, M, F):
    """FUNC bar against glue_ref.geglu_fwd / geglu_bwd; h, y, dy, dh are column slices with four different leading dimensions.
    E seen for these inputs (h ~ 2 N(0,1), dy ~ N(0,1)): forward 2.8e-6, backward 2.0e-6 at the wrap shape, 3e-7 .. 1e-6 at the small ones."""
    from vt355 import ops
    g = _gen(dev, 100 + M)
    h = _rand_in(M, 2 * F, 2 * F + 24, 8, dev, g, 2.0)
    dy = _rand_in(M, F, F + 40, 16, dev, g)
    ybuf, y = _slab(M, F, F + 8, 8, BF, dev)
    ops.geglu_fwd(h, y)
    ref = R.geglu_fwd(h.double())
    E = _func_error(R.geglu_fwd, [h])
    print(f"[geglu_fwd M={M} F={F}] fp32 evaluation error E = {E:.3g}")
    _within(y, ref, ULP * ref.abs() + 2 * E, "geglu_fwd")
    untouched(ybuf, _cols(8, F), "geglu_fwd")
    dbuf, dh = _slab(M, 2 * F, 2 * F + 16, 0, BF, dev)
    ops.geglu_bwd(dy, h, dh)
    ref = R.geglu_bwd(dy.double(), h.double())
    E = _func_error(R.geglu_bwd, [dy, h])
    print(f"[geglu_bwd M={M} F={F}] fp32 evaluation error E = {E:.3g}")
    _within(dh, ref, ULP * ref.abs() + 2 * E, "geglu_bwd")
    untouched(dbuf, _cols(0, 2 * F), "geglu_bwd")


@pytest.mark.parametrize("M,F", ROW_CASES)
def test_gated_gelu(dev, M, F):
    """FUNC bar against glue_ref.gated_gelu (tanh GELU); strided u and y.  E seen (u ~ 2 N(0,1)): 2.4e-6 at the wrap shape, 1.1e-6 and 1.6e-6 at the small ones."""
    from vt355 import ops
    g = _gen(dev, 200 + M)
    u = _rand_in(M, 2 * F, 2 * F + 8, 0, dev, g, 2.0)
    ybuf, y = _slab(M, F, F + 24, 16, BF, dev)
    ops.gated_gelu(u, y)
    ref = R.gated_gelu(u.double())
    E = _func_error(R.gated_gelu, [u])
    print(f"[gated_gelu M={M} F={F}] fp32 evaluation error E = {E:.3g}")
    _within(y, ref, ULP * ref.abs() + 2 * E, "gated_gelu")
    untouched(ybuf, _cols(16, F), "gated_gelu")


# ------------------------------------------------------------------ add_rows, residual_cast
@pytest.mark.parametrize("alias", ["none", "out_is_a", "out_is_b"])
@pytest.mark.parametrize("M,C", ROW_CASES)
def test_add_rows(dev, M, C, alias):
    """ONCE bar: bit-equal to the fp64 sum rounded once.  `out is a` and `out is b` are the calls hunyuan.py / unet.py make."""
    from vt355 import ops
    g = _gen(dev, 300 + M)
    a = _rand_in(M, C, C + 8, 0, dev, g, 3.0)
    b = _rand_in(M, C, C + 32, 24, dev, g, 0.05)
    want = _once(a.double() + b.double())
    if alias == "none":
        obuf, out = _slab(M, C, C + 16, 8, BF, dev)
        ops.add_rows(a, b, out)
        untouched(obuf, _cols(8, C), "add_rows")
    else:
        out = a if alias == "out_is_a" else b
        other = (b if alias == "out_is_a" else a).clone()
        ops.add_rows(a, b, out)
        _bits_equal(b if alias == "out_is_a" else a, other, "add_rows: the operand that is not the output")
        assert bool(is_poison(out._base)[:, C + (24 if alias == "out_is_b" else 0):].all()), "add_rows: pad columns of the aliased buffer"
    _bits_equal(out, want, f"add_rows ({alias})")


@pytest.mark.parametrize("lda_pad", [8, 4], ids=["lda%8==0", "lda%8==4"])
@pytest.mark.parametrize("with_r", [True, False], ids=["residual", "cast_only"])
@pytest.mark.parametrize("M,N", ROW_CASES)
def test_residual_cast(dev, M, N, with_r, lda_pad):
    """Without a residual this is the cast alone: bit-equal to acc.to(bf16) (MOVE / ONCE).  With one: fp32 acc + bf16 R in fp32, one bf16
    store -- ULP bar on |acc| + |R| (the fp32 sum of a 24-bit and an 8-bit value rounds before the bf16 store does)."""
    from vt355 import ops
    g = _gen(dev, 400 + M)
    acc = _rand_in(M, N, N + lda_pad, 4 if lda_pad == 4 else 8, dev, g, 2.0, F32)
    r = _rand_in(M, N, N + 16, 8, dev, g) if with_r else None
    obuf, out = _slab(M, N, N + 24, 16, BF, dev)
    ops.residual_cast(acc, r, out)
    if with_r:
        _within(out, acc.double() + r.double(), ULP * (acc.double().abs() + r.double().abs()), "residual_cast")
    else:
        _bits_equal(out, acc.to(BF), "residual_cast without a residual")
    untouched(obuf, _cols(16, N), "residual_cast")


# ------------------------------------------------------------------ dropout
def test_dropout_past_one_sweep_strided_and_in_place(dev):
    """Keep bits against oracle/philox.py on 24 sampled rows (first, last, and rows of the second sweep: chunk 4 194 304 starts in row
    16 320); the values are ONCE: x * (1 / (1 - p)) in fp32, one bf16 store, compared with that fp32 restatement; `y is x`; p = 0 keeps
    every element bit for bit."""
    import philox
    from vt355 import ops
    M, C = WIDE
    p, seed, off = 0.125, 2 ** 40 + 3, 7 << 36          # p exact in fp32: the kernel derives its threshold from the float
    g = _gen(dev, 500)
    x = _rand_in(M, C, C + 8, 8, dev, g)
    ybuf, y = _slab(M, C, C + 24, 16, BF, dev)
    mask = poisoned((M, C), torch.uint8, dev)
    ops.dropout(x, y, p, seed, off, mask_out=mask)
    assert not bool(is_poison(mask).any()) and bool((mask <= 1).all())
    rows = sorted(set([0, 1, M - 1, M - 2, 16319, 16320, 16321] + torch.randint(0, M, (17,), generator=torch.Generator().manual_seed(5)).tolist()))
    assert sum(r >= 16320 for r in rows) >= 4
    for r in rows:
        want = torch.from_numpy(philox.dropout_keep_mask(1, C, p, seed, off + r * C // 4))[0]
        assert torch.equal(mask[r].cpu(), want), f"dropout keep bits of row {r}"
    inv = torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))
    want = torch.where(mask.bool(), (x.float() * inv.to(dev)).to(BF), torch.zeros((), dtype=BF, device=dev))
    _bits_equal(y, want, "dropout values")
    untouched(ybuf, _cols(16, C), "dropout")
    assert abs(mask.float().mean().item() - (1 - p)) < 1e-3
    xin = x.clone()
    ops.dropout(x, x, p, seed, off)                                   # y may alias x
    _bits_equal(x, want, "dropout in place")
    assert bool(is_poison(x._base)[:, :8].all())
    y0 = poisoned((M, C), BF, dev)
    ops.dropout(xin, y0, 0.0, seed, off)
    _bits_equal(y0, xin, "dropout p = 0")


# ------------------------------------------------------------------ row_map
def _row_map_shapes(mode, nb, d1, d2):
    n = nb * d1 * d2
    return (4 * n if mode == 3 else n), (4 * n if mode in (1, 2) else n)


RM_WRAP = [tuple(R.sweep(f"vt_row_map_bf16 mode {m}")["shape"][k] for k in ("nb", "d1", "d2", "C")) for m in range(4)]
RM_CASES = [pytest.param(m, *RM_WRAP[m], id=f"mode{m}-wrap") for m in range(4)] + [
    pytest.param(0, 3, 1, 7, 24, id="mode0-d1=1"), pytest.param(0, 3, 7, 1, 24, id="mode0-d2=1"),
    pytest.param(3, 1, 82, 50, 4104, id="mode3-nb1"), pytest.param(1, 1, 1, 1, 8, id="mode1-one-row"), pytest.param(3, 2, 3, 5, 40, id="mode3-small")]


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("layout", ["contiguous", "strided"])
@pytest.mark.parametrize("mode,nb,d1,d2,C", RM_CASES)
def test_row_map(dev, mode, nb, d1, d2, C, layout, accumulate):
    """Modes 0-2 without accumulate are MOVE (bit-equal, zero rows of mode 2 included); mode 3 (a sum of four) and every accumulate
    (the map plus the known base) are ULP on the sum of the |terms|."""
    from vt355 import ops
    rs, ro = _row_map_shapes(mode, nb, d1, d2)
    g = _gen(dev, 600 + mode)
    lds, soff, ldo, ooff = (C, 0, C, 0) if layout == "contiguous" else (C + 8, 8, C + 24, 16)
    src = _rand_in(rs, C, lds, soff, dev, g)
    obuf, out = _slab(ro, C, ldo, ooff, BF, dev)
    base = None
    if accumulate:
        base = (torch.randn(ro, C, device=dev, generator=g) * 0.5).to(BF)
        out.copy_(base)
    ops.row_map(src, out, mode, nb, d1, d2, accumulate=accumulate)
    if mode < 3 and not accumulate:
        _bits_equal(out, R.row_map(src.contiguous(), mode, nb, d1, d2), f"row_map mode {mode}")
    else:
        ref = R.row_map(src.double(), mode, nb, d1, d2)
        terms = R.row_map_terms(src.double(), mode, nb, d1, d2)
        if accumulate:
            ref = ref + base.double(); terms = terms + base.double().abs()
        _within(out, ref, ULP * terms, f"row_map mode {mode} accumulate={accumulate}")
    untouched(obuf, _cols(ooff, C), f"row_map mode {mode}")


def test_row_map_mode0_twice_is_the_identity_and_mode3_is_the_gradient_of_mode1(dev):
    from vt355 import ops
    nb, d1, d2, C = RM_WRAP[0]
    g = _gen(dev, 650)
    src = _rand_in(nb * d1 * d2, C, C + 8, 0, dev, g)
    mid = poisoned((nb * d1 * d2, C), BF, dev); back = poisoned((nb * d1 * d2, C), BF, dev)
    ops.row_map(src, mid, 0, nb, d1, d2)
    ops.row_map(mid, back, 0, nb, d2, d1)
    _bits_equal(back, src, "row_map mode 0 twice")
    nb, d1, d2, C = 2, 5, 7, 24
    gy = (torch.randn(nb * 4 * d1 * d2, C, device=dev, generator=g)).to(BF)
    x = torch.zeros(nb, d1, d2, C, dtype=F64, device=dev, requires_grad=True)
    (x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).reshape(-1, C) * gy.double()).sum().backward()
    out = poisoned((nb * d1 * d2, C), BF, dev)
    ops.row_map(gy, out, 3, nb, d1, d2)
    _within(out, x.grad.view(-1, C), ULP * R.row_map_terms(gy.double(), 3, nb, d1, d2), "row_map mode 3 against autograd of mode 1")


# ------------------------------------------------------------------ gate_mul
_G = R.sweep("vt_gate_mul")["shape"]


@pytest.mark.parametrize("B,S,D,St", [pytest.param(_G["B"], _G["S"], _G["D"], _G["St"], id="wrap"), pytest.param(2, 50, 64, 0, id="St=0"),
                                      pytest.param(2, 50, 64, 50, id="St=S"), pytest.param(1, 50, 64, 7, id="B=1"), pytest.param(1, 1, 8, 0, id="M=1")])
def test_gate_mul(dev, B, S, D, St):
    """y = x * gate[sample, text-or-video] with both gates slices of one [B, 6 D] modulation table (bstride = 6 D), x and y column
    slices with different leading dimensions.  ONCE: bit-equal to the fp32 restatement (x.float() * gate).to(bf16) of the single
    multiplication (tests/test_glue_ref_cpu.py: a 24-bit gate can double-round against fp64, so fp64 is not the comparison here) --
    and within one bf16 ulp of the fp64 product as well."""
    from vt355 import ops
    g = _gen(dev, 700 + B * S)
    M = B * S
    x = _rand_in(M, D, D + 8, 0, dev, g)
    ybuf, y = _slab(M, D, D + 24, 8, BF, dev)
    table = torch.randn(B, 6 * D, device=dev, generator=g)
    g_txt, g_vid = table[:, 5 * D:], table[:, 2 * D:]
    ops.gate_mul(x, y, g_txt, g_vid, 6 * D, D, S, St)
    b, txt = R.gate_rows(M, S, St)
    gate = torch.where(txt.to(dev)[:, None], table[b.to(dev), 5 * D:6 * D], table[b.to(dev), 2 * D:3 * D])
    _bits_equal(y, (x.float() * gate).to(BF), "gate_mul")
    _within(y, x.double() * gate.double(), ULP * (x.double() * gate.double()).abs(), "gate_mul against fp64")
    untouched(ybuf, _cols(8, D), "gate_mul")


# ------------------------------------------------------------------ patchify / unpatchify
_P = R.sweep("vt_patchify")["shape"]


@pytest.mark.parametrize("B,Fr,C,H,W,P,pad", [pytest.param(_P["B"], _P["F"], _P["C"], _P["H"], _P["W"], _P["P"], 0, id="wrap"),
                                              pytest.param(2, 2, 3, 5, 7, 1, 0, id="P=1"), pytest.param(1, 2, 3, 8, 12, 4, 0, id="P=4"),
                                              pytest.param(2, 2, 16, 6, 10, 2, 24, id="ldt-padded")])
def test_patchify_unpatchify(dev, B, Fr, C, H, W, P, pad):
    """MOVE: bit-equal to glue_ref.patchify (columns (c p q), tokens (t h w)); pad columns of a wider token buffer stay untouched, and
    unpatchify reads the same strided buffer back to the source bits."""
    from vt355 import ops
    g = _gen(dev, 800 + P)
    img = torch.randn(B, Fr, C, H, W, device=dev, generator=g).to(BF)
    cols = C * P * P
    tbuf, tok = _slab(B * Fr * (H // P) * (W // P), cols, cols + pad, 0, BF, dev)
    ops.patchify(img, tok, P)
    _bits_equal(tok, R.patchify(img, P), "patchify")
    untouched(tbuf, _cols(0, cols), "patchify")
    back = poisoned(tuple(img.shape), BF, dev)
    ops.unpatchify(tok, back, P)
    _bits_equal(back, img, "unpatchify")
    tok2 = _rand_in(tok.shape[0], cols, cols + pad + 8, 8, dev, g)      # a token buffer that never was an image, strided differently
    back = poisoned(tuple(img.shape), BF, dev)
    ops.unpatchify(tok2, back, P)
    _bits_equal(back, R.unpatchify(tok2.contiguous(), B, Fr, C, H, W, P), "unpatchify from a strided tok")


# ------------------------------------------------------------------ timestep embedding
@pytest.mark.parametrize("shift", [0.0, 1.0])
@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("D", [2, 256, 320, 1920, 3072])
def test_timestep_embedding(dev, D, B, flip, shift):
    """FUNC bar against glue_ref.timestep_embedding in fp64: 2^-8 |ref| + max(2 E, |t| 2^-21) per row, E = max |fp32 evaluation - fp64|
    of the same formula on the CPU (seen: 3.0e-8 at D = 2, 3.1e-5 .. 6.9e-5 for D >= 256, all at t = 999, where the fp32 frequency's relative error is multiplied by
    the timestep; the |t| 2^-21 floor is the argument error of a 4-ulp expf).  D = 2 with freq_shift = 1 divides 0 by 0 in the reference
    formula as well: every output is then a NaN the kernel computed, not the poison."""
    from vt355 import ops
    t = torch.tensor([999] if B == 1 else [0, 1, 999, 500, 37])
    out = poisoned((B + 1, D), BF, dev)
    ops.timestep_embedding(t.to(dev), out[:B], flip, shift)
    untouched(out, slice(0, B), "timestep_embedding")
    if D == 2 and shift == 1.0:
        assert bool(torch.isnan(out[:B]).all()) and not bool(is_poison(out[:B]).any())
        return
    ref = R.timestep_embedding(t, D, flip, shift)
    E = (R.timestep_embedding(t, D, flip, shift, dtype=F32).double() - ref).abs().max().item()
    print(f"[timestep_embedding D={D} B={B} flip={flip} shift={shift}] fp32 evaluation error E = {E:.3g}")
    second = torch.maximum(torch.full((B, 1), 2 * E, dtype=F64), t.double().abs()[:, None] * 2.0 ** -21)
    _within(out[:B].cpu(), ref, ULP * ref.abs() + second, "timestep_embedding")


# ------------------------------------------------------------------ forward process
def _schedule(B, dev, g):
    sa = torch.rand(B, device=dev, generator=g) * 0.9 + 0.05
    return sa, (1 - sa * sa).sqrt()


@pytest.mark.parametrize("B,per", [pytest.param(R.sweep("vt_add_noise")["shape"]["B"], R.sweep("vt_add_noise")["shape"]["per"], id="wrap"), pytest.param(1, 1, id="one")])
def test_add_noise(dev, B, per):
    """ULP bar on |sa x0| + |sb eps| against glue_ref.add_noise"""
    from vt355 import ops
    g = _gen(dev, 900 + per)
    x0 = torch.randn(B, per, device=dev, generator=g); nz = torch.randn(B, per, device=dev, generator=g)
    sa, sb = _schedule(B, dev, g)
    out = poisoned((B * per + 8,), BF, dev)
    ops.add_noise(x0, nz, sa, sb, out[:B * per].view(B, per))
    ref = R.add_noise(x0.double(), nz.double(), sa, sb)
    terms = R.add_noise(x0.double().abs(), nz.double().abs(), sa, sb)
    _within(out[:B * per].view(B, per), ref, ULP * terms, "add_noise")
    untouched(out, slice(0, B * per), "add_noise")


@pytest.mark.parametrize("with_scale", [True, False], ids=["scale", "scale=None"])
@pytest.mark.parametrize("B,per", [pytest.param(R.sweep("vt_q_sample")["shape"]["B"], R.sweep("vt_q_sample")["shape"]["per"], id="wrap"), pytest.param(2, 3, id="tiny")])
def test_q_sample(dev, B, per, with_scale):
    """ULP bar on |sa scale x0| + |sb eps| against glue_ref.q_sample"""
    from vt355 import ops
    g = _gen(dev, 1000 + per)
    x0 = torch.randn(B, per, device=dev, generator=g); nz = torch.randn(B, per, device=dev, generator=g)
    sa, sb = _schedule(B, dev, g)
    sc = (torch.rand(B, device=dev, generator=g) + 0.5) if with_scale else None
    out = poisoned((B * per + 8,), BF, dev)
    ops.q_sample(x0, nz, sa, sb, sc, out[:B * per].view(B, per))
    ref = R.q_sample(x0.double(), nz.double(), sa, sb, sc)
    terms = R.q_sample(x0.double().abs(), nz.double().abs(), sa, sb, sc)
    _within(out[:B * per].view(B, per), ref, ULP * terms, "q_sample")
    untouched(out, slice(0, B * per), "q_sample")


# ------------------------------------------------------------------ losses
def test_diffusion_loss_and_bwd_past_one_sweep(dev):
    """loss: the project's 1e-4 relative bar of the fp32 losses (tests/test_kernels_gpu.py).  dvpred: ULP bar on the |terms| of
    x0_hat - x0 times the factor in front (glue_ref.diffusion_loss_grad).  The weights differ by 10^4 between the samples, so a sample
    index taken wrong after the first sweep (131 072 elements; sample 1 starts at 100 003) is far outside either bar."""
    from vt355 import ops
    s = R.sweep("vt_diffusion_loss")["shape"]
    B, per = s["B"], s["per"]
    g = _gen(dev, 1100)
    x0 = torch.randn(B, per, device=dev, generator=g); nz = torch.randn(B, per, device=dev, generator=g)
    sa = torch.tensor([0.95, 0.6, 0.2], device=dev); sb = (1 - sa * sa).sqrt()
    w = torch.tensor([100.0, 1.0, 0.01], device=dev)
    noisy = R.add_noise(x0, nz, sa, sb).to(BF)
    vp = torch.randn(B, per, device=dev, generator=g).to(BF)
    args = (vp, noisy, x0, sa, sb, w)
    ref_loss = R.diffusion_loss(vp.double(), noisy.double(), x0.double(), sa, sb, w).item()
    grad, terms = R.diffusion_loss_grad(vp.double(), noisy.double(), x0.double(), sa, sb, w)
    gs = torch.tensor(0.37, dtype=F32).item()
    losses = []
    for scale in (1.0, gs):
        loss = poisoned((1,), F32, dev); part = poisoned((512,), F32, dev); dv = poisoned((B * per + 8,), BF, dev)
        ops.diffusion_loss(*args, loss, part, dv[:B * per].view(B, per), scale)
        assert abs(loss.item() - ref_loss) <= 1e-4 * abs(ref_loss), (loss.item(), ref_loss)
        _within(dv[:B * per].view(B, per), grad * scale, ULP * terms * scale, f"diffusion_loss dvpred, grad_scale {scale}")
        untouched(dv, slice(0, B * per), "diffusion_loss dvpred")
        losses.append(loss.clone())
    loss = poisoned((1,), F32, dev); part = poisoned((512,), F32, dev)
    ops.diffusion_loss(*args, loss, part, None, 1.0)
    _bits_equal(loss, losses[0], "diffusion_loss with dvpred = None")          # no atomics: the same sum in the same order
    _bits_equal(losses[1], losses[0], "diffusion_loss: grad_scale must not touch the loss")
    for go in (1.0, gs):
        dv = poisoned((B * per + 8,), BF, dev)
        ops.diffusion_loss_bwd(*args, torch.tensor([go], device=dev), dv[:B * per].view(B, per))
        _within(dv[:B * per].view(B, per), grad * go, ULP * terms * go, f"diffusion_loss_bwd, grad_out {go}")
        untouched(dv, slice(0, B * per), "diffusion_loss_bwd")


@pytest.mark.parametrize("with_dpred", [True, False], ids=["dpred", "dpred=None"])
def test_mse_loss_past_one_sweep(dev, with_dpred):
    """loss at the 1e-4 relative bar only (float atomics reorder the sum); dpred: ULP bar on (|pred| + |target|) * 2 gscale / n, and the
    same bits from a second launch"""
    from vt355 import ops
    s = R.sweep("vt_mse_loss")["shape"]
    B, per = s["B"], s["per"]
    g = _gen(dev, 1200)
    pred = torch.randn(B, per, device=dev, generator=g).to(BF); tgt = torch.randn(B, per, device=dev, generator=g)
    ref = R.mse_loss(pred.double(), tgt.double()).item()
    gs = 0.5
    loss = poisoned((1,), F32, dev)
    dp = poisoned((B * per + 8,), BF, dev) if with_dpred else None
    ops.mse_loss(pred, tgt, loss, dp[:B * per].view(B, per) if with_dpred else None, grad_scale=gs)
    assert abs(loss.item() - ref) <= 1e-4 * abs(ref), (loss.item(), ref)
    if with_dpred:
        grad, terms = R.mse_loss_grad(pred.double(), tgt.double())
        _within(dp[:B * per].view(B, per), grad * gs, ULP * terms * gs, "mse_loss dpred")
        untouched(dp, slice(0, B * per), "mse_loss dpred")
        dp2 = poisoned((B * per,), BF, dev); loss2 = poisoned((1,), F32, dev)
        ops.mse_loss(pred, tgt, loss2, dp2.view(B, per), grad_scale=gs)
        _bits_equal(dp2, dp[:B * per], "mse_loss dpred of a second launch")
        assert abs(loss2.item() - ref) <= 1e-4 * abs(ref)


def test_opensora_loss_past_one_sweep(dev):
    """loss3 at the bars of tests/test_stdit_gpu.py::test_opensora_loss_kernel_matches_golden (1e-6 relative for loss and vb, 1e-5 for
    mse) against glue_ref.opensora_loss in fp64; dout against its autograd gradient: the kernel computes in fp64 and stores fp32, so
    2^-23 |ref| (the store, with a factor 2) + 1e-9 max|ref| (fp64 evaluation differences of tanh / exp / log, amplified where
    cdf_plus - cdf_minus cancels; the inputs keep that difference above 1e-3).  Sample 0 has t = 0 (discretised-Gaussian branch), sample 1
    t = 500 (KL branch); a tenth of the x0 entries lie beyond +-0.999, so all three likelihood branches run."""
    from vt355 import ops
    from vt355.stdit import OpenSoraScheduler
    s = R.sweep("vt_opensora_loss")["shape"]
    B, C, per = s["B"], s["C"], s["per_c"]
    g = _gen(dev, 1300)
    x0 = (torch.randn(B, C, per, device=dev, generator=g) * 0.6).clamp(-1.3, 1.3)
    nz = torch.randn(B, C, per, device=dev, generator=g)
    out = torch.randn(B, 2 * C, per, device=dev, generator=g) * 0.7
    out[0, :C] = x0[0] + 0.002 * torch.randn(C, per, device=dev, generator=g)      # t = 0: mean_p = eps_hat; keep |z| moderate
    coef = OpenSoraScheduler().coef(torch.tensor([0, 500], device=dev))
    assert coef[0, 6].item() == 1.0 and coef[1, 6].item() == 0.0
    assert int((x0[0] < -0.999).sum()) > 100 and int((x0[0] > 0.999).sum()) > 100
    loss3 = poisoned((3,), F64, dev); dout = poisoned((B * 2 * C * per + 8,), F32, dev)
    ops.opensora_loss(out, x0, nz, coef, loss3, dout[:out.numel()].view(out.shape))
    o = out.double().requires_grad_(True)
    ref = R.opensora_loss(o, x0.double(), nz.double(), coef)
    ref[0].backward()
    for i, (name, bar) in enumerate((("loss", 1e-6), ("mse", 1e-5), ("vb", 1e-6))):
        assert abs(loss3[i].item() - ref[i].item()) <= bar * abs(ref[i].item()), (name, loss3[i].item(), ref[i].item())
    _within(dout[:out.numel()].view(out.shape), o.grad, 2.0 ** -23 * o.grad.abs() + 1e-9 * o.grad.abs().max().item(), "opensora_loss dout")
    untouched(dout, slice(0, out.numel()), "opensora_loss dout")
    l2 = poisoned((3,), F64, dev)
    ops.opensora_loss(out, x0, nz, coef, l2, None)
    assert abs(l2[0].item() - loss3[0].item()) <= 1e-12 * abs(loss3[0].item())


# ------------------------------------------------------------------ AdamW
def _f32(x):
    return torch.tensor(x, dtype=F32).item()


HYPER = {"defaults": dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2), "custom": dict(lr=1e-4, b1=0.95, b2=0.99, eps=1e-6, wd=0.1),
         "wd=0": dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0)}
N_WRAP = R.sweep("vt_adamw")["shape"]["n"]


def _adamw_inputs(n, dev, g):
    """|p| in [1e-3, 1]; every element keeps ONE gradient sign over the steps (m then has no cancellation, which its relative bar would
    charge to the kernel); the magnitudes are redrawn each step from 1e-9 .. 1, mixed within the buffer"""
    sign = lambda: torch.where(torch.rand(n, device=dev, generator=g) < 0.5, -1.0, 1.0)
    p = sign() * 10.0 ** (-3.0 * torch.rand(n, device=dev, generator=g))
    gsign = sign()
    grad = lambda: gsign * 10.0 ** (-9.0 * torch.rand(n, device=dev, generator=g))
    return p, grad


@pytest.mark.parametrize("hyper", list(HYPER))
@pytest.mark.parametrize("n", [N_WRAP, 1, 257])
def test_adamw_state_and_update(dev, n, hyper):
    """Steps 1, 2, 3 and then step = 5000 on the carried state, against glue_ref.adamw_step in fp64 fed the SAME fp32 inputs (state,
    gradient, hyper-parameters as the fp32 values the C ABI passes).  Bars from counting fp32 roundings (2^-24 relative each):
      m, v     at most four (two products, one sum, one more product in v): 2^-22 relative;
      update   p_old (1 - lr wd) - p_new: three roundings on the scale of p (1 - lr wd, the product, the final difference), 2^-22 |p_old|,
               plus at most 16 inside lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps): 2^-20 |update|.
    With |g| from 1e-9 to 1 the term eps weighs anything between nothing and everything in the denominator, so eps on the wrong side of
    the sqrt(bc2) division, or decay after the step, are far outside the second term."""
    from vt355 import ops
    hp = {k: _f32(v) for k, v in HYPER[hyper].items()}
    g = _gen(dev, 1400 + n % 1000)
    p0, grad = _adamw_inputs(n, dev, g)
    p = p0.clone(); m = torch.zeros(n, device=dev); v = torch.zeros(n, device=dev)
    pb = poisoned((n + 8,), BF, dev)
    for step in (1, 2, 3, 5000):
        gr = grad()
        p_old, m_old, v_old = p.double(), m.double(), v.double()
        ops.adamw(p, gr, m, v, pb[:n], hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], step)
        _, m_ref, v_ref, upd_ref = R.adamw_step(p_old, gr.double(), m_old, v_old, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], step)
        _within(m, m_ref, 2.0 ** -22 * m_ref.abs(), f"adamw m, step {step}")
        _within(v, v_ref, 2.0 ** -22 * v_ref.abs(), f"adamw v, step {step}")
        upd = p_old * (1.0 - hp["lr"] * hp["wd"]) - p.double()
        _within(upd, upd_ref, 2.0 ** -22 * p_old.abs() + 2.0 ** -20 * upd_ref.abs(), f"adamw update, step {step}")
        _bits_equal(pb[:n], p.to(BF), f"adamw p_bf16, step {step}")
        untouched(pb, slice(0, n), "adamw p_bf16")


@pytest.mark.parametrize("n", [257, N_WRAP])
def test_adamw_grad_scale_guard_and_no_bf16_copy(dev, n):
    """grad_scale = 1/8 on gradients times 8 gives the bits of grad_scale = 1 (a power of two scales exactly); p_bf16 = None changes
    nothing else; guard = 1 leaves p, m, v, p_bf16 bit for bit as they were; guard = 0 equals guard = None."""
    from vt355 import ops
    hp = {k: _f32(v) for k, v in HYPER["custom"].items()}
    g = _gen(dev, 1500)
    p0, grad = _adamw_inputs(n, dev, g)
    gr = grad()
    m0 = gr * 0.3; v0 = gr * gr * 0.2

    def run(grads, gscale, guard, with_pb=True):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        pb = poisoned((n,), BF, dev) if with_pb else None
        ops.adamw(p, grads, m, v, pb, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], 7, grad_scale=gscale, guard=guard)
        return p, m, v, pb

    base = run(gr, 1.0, None)
    assert not bool(torch.equal(base[0], p0))
    for name, other in (("grad_scale 1/8", run(gr * 8.0, 0.125, None)), ("guard = 0", run(gr, 1.0, torch.zeros(1, dtype=torch.int32, device=dev)))):
        for a, b, what in zip(base, other, "p m v p_bf16".split()):
            _bits_equal(b, a, f"adamw {name}: {what}")
    nopb = run(gr, 1.0, None, with_pb=False)
    for a, b, what in zip(base[:3], nopb[:3], "p m v".split()):
        _bits_equal(b, a, f"adamw p_bf16 = None: {what}")
    held = run(gr, 1.0, torch.ones(1, dtype=torch.int32, device=dev))
    for a, b, what in zip((p0, m0, v0), held[:3], "p m v".split()):
        _bits_equal(b, a, f"adamw guard = 1: {what}")
    assert bool(is_poison(held[3]).all()), "adamw guard = 1 wrote p_bf16"


# ------------------------------------------------------------------ the wrappers refuse operands smaller than the launch
# In every test the short operand is a NARROW VIEW of a poisoned allocation large enough for the whole launch: a wrapper that failed to
# refuse would still stay inside memory the test owns.  After the refusal the allocation is still poison from end to end.
def _refused(buf, call, match):
    with pytest.raises(ValueError, match=match):
        call()
    torch.cuda.synchronize()
    assert bool(is_poison(buf).all()), f"{match}: the refused call wrote"


def test_geglu_fwd_refuses_a_short_output(dev):
    from vt355 import ops
    h = torch.zeros(16, 32, dtype=BF, device=dev); y = poisoned((16, 16), BF, dev)
    _refused(y, lambda: ops.geglu_fwd(h, y[:15]), "geglu_fwd")
    _refused(y, lambda: ops.geglu_fwd(h, y[:, :8]), "geglu_fwd")


def test_geglu_bwd_refuses_short_operands(dev):
    from vt355 import ops
    h = torch.zeros(16, 32, dtype=BF, device=dev); dy = torch.zeros(16, 16, dtype=BF, device=dev); dh = poisoned((16, 32), BF, dev)
    _refused(dh, lambda: ops.geglu_bwd(dy, h, dh[:15]), "geglu_bwd")
    _refused(dh, lambda: ops.geglu_bwd(dy[:15], h, dh), "geglu_bwd")
    _refused(dh, lambda: ops.geglu_bwd(dy[:, :8], h, dh), "geglu_bwd")


def test_add_rows_refuses_short_operands(dev):
    from vt355 import ops
    a = torch.zeros(16, 16, dtype=BF, device=dev); out = poisoned((16, 16), BF, dev)
    _refused(out, lambda: ops.add_rows(a, a, out[:15]), "add_rows")
    _refused(out, lambda: ops.add_rows(a, a[:15], out), "add_rows")
    _refused(out, lambda: ops.add_rows(a, a, out[:, :8]), "add_rows")


def test_dropout_refuses_a_short_output(dev):
    from vt355 import ops
    x = torch.zeros(16, 16, dtype=BF, device=dev); y = poisoned((16, 16), BF, dev)
    _refused(y, lambda: ops.dropout(x, y[:15], 0.1, 1), "dropout")
    _refused(y, lambda: ops.dropout(x, y[:, :8], 0.1, 1), "dropout")


def test_gate_mul_refuses_short_operands(dev):
    from vt355 import ops
    B, S, D = 3, 4, 16
    x = torch.zeros(B * S, D, dtype=BF, device=dev); y = poisoned((B * S, D), BF, dev)
    table = torch.ones(B, 6 * D, device=dev)
    gate = table[:, 2 * D:3 * D]
    _refused(y, lambda: ops.gate_mul(x, y[:B * S - 1], gate, gate, 6 * D, D, S, 0), "gate_mul")
    _refused(y, lambda: ops.gate_mul(x, y, gate[:B - 1], gate, 6 * D, D, S, 0), "gate_mul")
    _refused(y, lambda: ops.gate_mul(x, y, gate, gate[:, :D - 8], 6 * D, D, S, 0), "gate_mul")
    _refused(y, lambda: ops.gate_mul(x, y, gate, table[0, :D], 6 * D, D, S, 0), "gate_mul")


def test_add_noise_refuses_short_operands(dev):
    from vt355 import ops
    B, per = 3, 40
    x0 = torch.zeros(B, per, device=dev); vec = torch.ones(B, device=dev); out = poisoned((B, per), BF, dev)
    _refused(out, lambda: ops.add_noise(x0, x0, vec, vec, out[:B - 1]), "add_noise")
    _refused(out, lambda: ops.add_noise(x0, x0[:B - 1], vec, vec, out), "add_noise")
    _refused(out, lambda: ops.add_noise(x0, x0, vec[:B - 1], vec, out), "add_noise")
    _refused(out, lambda: ops.add_noise(x0, x0, vec, vec[:B - 1], out), "add_noise")


def test_q_sample_refuses_short_operands(dev):
    from vt355 import ops
    B, per = 3, 40
    x0 = torch.zeros(B, per, device=dev); vec = torch.ones(B, device=dev); out = poisoned((B, per), BF, dev)
    _refused(out, lambda: ops.q_sample(x0, x0, vec, vec, None, out[:B - 1]), "q_sample")
    _refused(out, lambda: ops.q_sample(x0, x0[:B - 1], vec, vec, None, out), "q_sample")
    _refused(out, lambda: ops.q_sample(x0, x0, vec, vec[:B - 1], vec, out), "q_sample")
    _refused(out, lambda: ops.q_sample(x0, x0, vec, vec, vec[:B - 1], out), "q_sample")


def test_mse_loss_refuses_short_operands(dev):
    from vt355 import ops
    pred = torch.zeros(3, 40, dtype=BF, device=dev); tgt = torch.zeros(3, 40, device=dev)
    dp = poisoned((3, 40), BF, dev); loss = poisoned((1,), F32, dev)
    _refused(dp, lambda: ops.mse_loss(pred, tgt, loss, dp[:2]), "mse_loss")
    _refused(dp, lambda: ops.mse_loss(pred, tgt[:2], loss, dp), "mse_loss")
    assert bool(is_poison(loss).all())


def test_diffusion_loss_refuses_short_operands(dev):
    from vt355 import ops
    B, per = 3, 40
    vp = torch.zeros(B, per, dtype=BF, device=dev); x0 = torch.zeros(B, per, device=dev); vec = torch.ones(B, device=dev)
    loss = poisoned((1,), F32, dev); part = poisoned((512,), F32, dev); dv = poisoned((B, per), BF, dev)
    for bad in (lambda: ops.diffusion_loss(vp, vp, x0, vec, vec, vec, loss, part[:511], dv),
                lambda: ops.diffusion_loss(vp, vp, x0, vec, vec, vec, loss, part, dv[:B - 1]),
                lambda: ops.diffusion_loss(vp[:B - 1], vp, x0, vec, vec, vec, loss, part, dv),
                lambda: ops.diffusion_loss(vp, vp, x0, vec, vec, vec[:B - 1], loss, part, dv)):
        _refused(dv, bad, "diffusion_loss")
        assert bool(is_poison(part).all()) and bool(is_poison(loss).all())


def test_diffusion_loss_bwd_refuses_short_operands(dev):
    from vt355 import ops
    B, per = 3, 40
    vp = torch.zeros(B, per, dtype=BF, device=dev); x0 = torch.zeros(B, per, device=dev); vec = torch.ones(B, device=dev)
    go = torch.ones(1, device=dev); dv = poisoned((B, per), BF, dev)
    _refused(dv, lambda: ops.diffusion_loss_bwd(vp, vp, x0, vec, vec, vec, go, dv[:B - 1]), "diffusion_loss_bwd")
    _refused(dv, lambda: ops.diffusion_loss_bwd(vp, vp[:B - 1], x0, vec, vec, vec, go, dv), "diffusion_loss_bwd")
    _refused(dv, lambda: ops.diffusion_loss_bwd(vp, vp, x0, vec[:B - 1], vec, vec, go, dv), "diffusion_loss_bwd")
    _refused(dv, lambda: ops.diffusion_loss_bwd(vp, vp, x0, vec, vec, vec, go[:0], dv), "diffusion_loss_bwd")


def test_patchify_refuses_a_wrong_token_count(dev):
    from vt355 import ops
    B, Fr, C, H, W, P = 1, 2, 3, 4, 6, 2
    img = torch.zeros(B, Fr, C, H, W, dtype=BF, device=dev)
    rows = B * Fr * (H // P) * (W // P)
    tok = poisoned((rows, C * P * P), BF, dev)
    _refused(tok, lambda: ops.patchify(img, tok[:rows - 1], P), "patchify")


def test_unpatchify_refuses_a_wrong_token_count(dev):
    from vt355 import ops
    B, Fr, C, H, W, P = 1, 2, 3, 4, 6, 2
    rows = B * Fr * (H // P) * (W // P)
    out = poisoned((B, Fr, C, H, W), BF, dev)
    src = torch.zeros(rows, C * P * P, dtype=BF, device=dev)
    _refused(out, lambda: ops.unpatchify(src[:rows - 1], out, P), "unpatchify")


# ------------------------------------------------------------------ C-side guards
def test_abi_rejects_bad_glue_arguments(dev):
    """The library's own guards of the glue entry points: each refuses on the host with a code the binding turns into VtError naming the
    entry point, and nothing is written."""
    from vt355 import ops
    from vt355._lib import VtError
    out = poisoned((16, 64), BF, dev)
    a = torch.zeros(18, 64, dtype=BF, device=dev)[:16]               # two spare rows: every refused call would stay inside them
    acc = torch.zeros(16, 64, device=dev)
    lap = lambda t: torch.as_strided(t, (16, 16), (8, 1))            # rows that overlap: ld = 8 < C = 16
    gate = torch.ones(1, 64, device=dev)

    def refused(match, call):
        with pytest.raises(VtError, match=match):
            call()
        torch.cuda.synchronize()
        assert bool(is_poison(out).all()), f"{match}: the refused call wrote"

    odd = torch.zeros(16, 68, dtype=BF, device=dev)                   # ld = 68: not a multiple of 8
    refused("vt_add_rows_bf16", lambda: ops.add_rows(a[:, :12], a[:, :12], out[:, :12]))                  # C % 8
    refused("vt_add_rows_bf16", lambda: ops.add_rows(odd[:, :16], a[:, :16], out[:, :16]))               # ld % 8
    refused("vt_add_rows_bf16", lambda: ops.add_rows(a[:, 4:20], a[:, :16], out[:, :16]))                # misaligned base
    refused("vt_geglu_fwd", lambda: ops.geglu_fwd(a[:, :24], out[:, :12]))                                # F % 8
    refused("vt_geglu_fwd", lambda: ops.geglu_fwd(odd[:, :32], out[:, :16]))
    refused("vt_geglu_bwd", lambda: ops.geglu_bwd(a[:, 4:20], a[:, :32], out[:, :32]))
    refused("vt_gated_gelu_bf16", lambda: ops.gated_gelu(a[:, :24], out[:, :12]))
    refused("vt_gated_gelu_bf16", lambda: ops.gated_gelu(a[:, :40], out[:, :40]))                        # ldu = 64 < 2 F = 80
    refused("vt_add_rows_bf16", lambda: ops.add_rows(a[:, :16], a[:, :16], lap(out)))                    # ld < C
    refused("vt_add_rows_bf16", lambda: ops.add_rows(lap(a), a[:, :16], out[:, :16]))
    refused("vt_geglu_fwd", lambda: ops.geglu_fwd(a[:, :32], lap(out)))
    refused("vt_dropout_bf16", lambda: ops.dropout(a[:, :16], lap(out), 0.1, 1))
    refused("vt_row_map_bf16", lambda: ops.row_map(a[:, :16], lap(out), 0, 1, 4, 4))
    refused("vt_residual_cast_bf16", lambda: ops.residual_cast(acc[:, :16], None, lap(out)))
    refused("vt_residual_cast_bf16", lambda: ops.residual_cast(acc[:, :12], None, out[:, :12]))
    refused("vt_residual_cast_bf16", lambda: ops.residual_cast(acc[:, 1:17], None, out[:, :16]))         # misaligned fp32 base
    refused("vt_residual_cast_bf16", lambda: ops.residual_cast(acc[:, :16], odd[:, :16], out[:, :16]))
    refused("vt_dropout_bf16", lambda: ops.dropout(a[:, :12], out[:, :12], 0.1, 1))
    refused("vt_dropout_bf16", lambda: ops.dropout(a[:, :16], out[:, :16], 1.0, 1))                      # p must be below 1
    refused("vt_row_map_bf16", lambda: ops.row_map(a, out, 4, 1, 4, 4))                                   # mode 4
    refused("vt_row_map_bf16", lambda: ops.row_map(a[:, :12], out[:, :12], 0, 1, 4, 4))
    refused("vt_row_map_bf16", lambda: ops.row_map(odd[:, :16], out[:, :16], 0, 1, 4, 4))
    refused("vt_row_map_bf16", lambda: ops.row_map(a[:, 4:20], out[:, :16], 0, 1, 4, 4))
    refused("vt_gate_mul", lambda: ops.gate_mul(a[:, :12], out[:, :12], gate, gate, 64, 12, 16, 0))
    refused("vt_gate_mul", lambda: ops.gate_mul(odd[:, :16], out[:, :16], gate, gate, 64, 16, 16, 0))
    refused("vt_gate_mul", lambda: ops.gate_mul(a[:, 4:20], out[:, :16], gate, gate, 64, 16, 16, 0))
    refused("vt_gate_mul", lambda: ops.gate_mul(a[:, :16], out[:, :16], gate[:, 1:], gate, 64, 16, 16, 0))   # misaligned gate
    img = torch.zeros(1, 1, 2, 6, 4, dtype=BF, device=dev)
    refused("vt_patchify", lambda: ops.patchify(img, out, 4))                                             # H % P
    refused("vt_unpatchify", lambda: ops.unpatchify(a, poisoned((1, 1, 2, 4, 6), BF, dev), 4))          # W % P
    refused("vt_patchify", lambda: ops.patchify(img, out.view(-1)[:24].view(6, 4), 2))                    # ldt = 4 < C P P = 8
    refused("vt_timestep_embedding", lambda: ops.timestep_embedding(torch.zeros(16, dtype=torch.int64, device=dev), out[:, :63]))   # D odd
    p = torch.zeros(64, device=dev)
    refused("vt_adamw", lambda: ops.adamw(p, p, p, p, out.view(-1)[:64], 1e-3, 0.9, 0.999, 1e-8, 0.0, 0))   # step = 0
    refused("vt_adamw_clip", lambda: ops.adamw(p, p, p, p, out.view(-1)[:64], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, clip_coef=torch.ones(1, device=dev),
                                               clip_value=1.0))                                          # one clip algorithm per step
    assert float(p.abs().max()) == 0.0
