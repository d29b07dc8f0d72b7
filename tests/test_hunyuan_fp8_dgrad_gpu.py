"""HunyuanVideo fp8="mfma" with fp8_dgrad: the input-gradient products dX = g W on the MX-scaled fp8 matrix cores.  Kernels first
(vt_gemm_mxfp8_dx, vt_gate_mul_fp8, vt_cast_fp8_fmt, vt_fp8_scale_update_fmax) against references computed from the de-quantised
operands, then the mode in HunyuanBlocks / HYVideoDiffusionTransformer against fp8="mfma" alone (its bf16 backward)."""
import pytest
import torch

from parity import all_written, cosine, poisoned, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
FMAX = {E4: 448.0, E5: 57344.0}
FMTS = [pytest.param(E5, id="e5m2"), pytest.param(E4, id="e4m3")]


def _fp8_cpu(x_bf16, scale, dt):
    """satfinite(RNE(x / scale)) on the CPU: clamp first (an unclamped cast to float8_e5m2 overflows to inf), IEEE division"""
    return (x_bf16.float().cpu() / scale.float().cpu()).clamp(-FMAX[dt], FMAX[dt]).to(dt)


def _bytes(t):
    return t.cpu().view(torch.uint8)


def _gelu_tanh_grad(x):
    c = 0.7978845608028654
    t = torch.tanh(c * (x + 0.044715 * x ** 3))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * c * (1.0 + 3.0 * 0.044715 * x * x)


@pytest.mark.parametrize("gfmt", FMTS)
@pytest.mark.parametrize("M,N,K", [(128, 128, 128), (300, 260, 384)])
def test_gemm_mxfp8_dx_lane_map_exact(dev, M, N, K, gfmt):
    """integers -7 .. 7 are exact in E5M2 and in E4M3, their fp32 sums exact: the result must equal the integer product rounded once to
    bf16.  The gradient (E5M2 or E4M3) and the transposed weight (always E4M3, two planted asymmetric entries) are independent random
    integers, so a format code in the wrong operand slot (the same bytes decode to other numbers), a swapped row / column map or a
    disagreement on the k order cannot pass; ragged M and N exercise the edge tiles; power-of-two scales keep it exact"""
    from vt355 import ops
    gen = torch.Generator().manual_seed(1)
    g = torch.randint(-7, 8, (M, K), generator=gen).float()
    w = torch.randint(-3, 4, (N, K), generator=gen).float()
    w[0, 0], w[1, K - 1] = 7.0, -6.0
    assert torch.equal(g.to(gfmt).float(), g) and torch.equal(w.to(E4).float(), w)
    gq, wq = g.to(gfmt).to(dev), w.to(E4).to(dev)
    sg = torch.tensor([0.5], device=dev); sw = torch.tensor([4.0], device=dev)
    out = torch.full((M, N), 3.0, dtype=BF, device=dev)
    ops.gemm_mxfp8_dx(gq, wq, out, sg, sw)
    ref = ((g.double() @ w.double().t()) * 2.0).to(BF)
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("gfmt", FMTS)
@pytest.mark.parametrize("which", ["linear1 columns", "linear2 rows"])
def test_gemm_mxfp8_dx_sliced_weight_exact(dev, which, gfmt):
    """the weight operand as the model hands it over for the single blocks: a COLUMN slice of a wider transposed weight (linear1's row
    ranges: ldw > K, base pointer c0 bytes into the row) or a ROW slice of a taller one (linear2's column ranges: base pointer r0 rows
    in), the output a column range of a wider buffer.  Exact integers as above, every entry outside the slice set to a value that would
    change the result if it were read, ragged M and N: torch.equal to the integer product"""
    from vt355 import ops
    gen = torch.Generator().manual_seed(7)
    M = 200
    if which == "linear1 columns":
        R, C, r0, c0, N, K = 260, 640, 0, 256, 260, 384         # wqt[:, 256:640] of [260, 640]
    else:
        R, C, r0, c0, N, K = 516, 256, 128, 0, 388, 256         # wqt[128:516] of [516, 256]
    g = torch.randint(-7, 8, (M, K), generator=gen).float()
    full = torch.full((R, C), 5.0)
    w = torch.randint(-3, 4, (N, K), generator=gen).float()
    w[0, 0], w[1, K - 1] = 7.0, -6.0
    full[r0:r0 + N, c0:c0 + K] = w
    gq, wfull = g.to(gfmt).to(dev), full.to(E4).to(dev)
    wq = wfull[r0:r0 + N, c0:c0 + K]
    assert wq.stride(0) == C and wq.data_ptr() == wfull.data_ptr() + r0 * C + c0
    sg = torch.tensor([0.25], device=dev); sw = torch.tensor([2.0], device=dev)
    buf = torch.full((M, N + 128), 3.0, dtype=BF, device=dev)
    ops.gemm_mxfp8_dx(gq, wq, buf[:, 128:], sg, sw)
    ref = ((g.double() @ w.double().t()) * 0.5).to(BF)
    assert torch.equal(buf[:, 128:].cpu(), ref) and bool((buf[:, :128] == 3.0).all())


def _quant_w(x, dev):
    from vt355 import ops
    xq, s = ops.quantize_fp8(x.to(dev, BF).contiguous())
    return xq, s, xq.double().cpu() * s.double().cpu()


def _quant_g(x, dt, dev):
    """a gradient quantised per tensor on the CPU: (gq on the device, scale on the device, the de-quantised values in fp64)"""
    xb = x.to(BF)
    s = (xb.float().abs().max() / FMAX[dt]).reshape(1)
    q = _fp8_cpu(xb, s, dt)
    return q.to(dev), s.to(dev), q.double() * s.double()


_SMALL = [(e, t, 200, 384, 256) for e in ("plain", "dgelu", "res") for t in (False, True)]
_FULL = [("plain", False, 10456, 3072, 9216), ("dgelu", True, 10456, 12288, 3072)]        # one full block shape per epilogue with a full shape


@pytest.mark.parametrize("gfmt", FMTS)
@pytest.mark.parametrize("epi,tail,M,N,K", _SMALL + _FULL)
def test_gemm_mxfp8_dx_random_vs_fp64(dev, epi, tail, M, N, K, gfmt):
    """random operands vs fp64 of the DE-QUANTISED operands (no tolerance absorbs quantisation): plain store, dGELU with a saved
    pre-activation, + residual; with and without the 64-column bf16 tail; gradient in E5M2 and in E4M3.  Only the bf16 rounding of the
    output is left: the cap is test_gemm_mxfp8_random_vs_fp64's 5e-3.  Measured rel-L2 (MI355X): 1.65e-3 .. 1.67e-3 in every case, printed"""
    from vt355 import ops
    from vt355.ops import EPI_DGELU, EPI_GATED_RES
    gen = torch.Generator().manual_seed(2)
    gq, sg, gd = _quant_g(torch.randn(M, K, generator=gen), gfmt, dev)
    wq, sw, wd = _quant_w(torch.randn(N, K, generator=gen) * K ** -0.5, dev)
    ref = (gd.to(dev) @ wd.to(dev).t()).cpu()
    kw = {}
    if tail:
        At = (torch.randn(M, 64, generator=gen) * 0.5).to(BF); Wt = (torch.randn(N, 64, generator=gen) * 0.1).to(BF)
        ref = ref + At.double() @ Wt.double().t()
        kw["tail"] = (At.to(dev), Wt.to(dev))
    out = poisoned((M, N), BF, dev)
    if epi == "plain":
        ops.gemm_mxfp8_dx(gq, wq, out, sg, sw, **kw)
    elif epi == "dgelu":
        u = torch.randn(M, N, generator=gen).to(BF)
        ops.gemm_mxfp8_dx(gq, wq, out, sg, sw, epilogue=EPI_DGELU, pre_act_in=u.to(dev), **kw)
        ref = ref * _gelu_tanh_grad(u.double())
    else:
        R = torch.randn(M, N, generator=gen).to(BF)
        ops.gemm_mxfp8_dx(gq, wq, out, sg, sw, epilogue=EPI_GATED_RES, residual=R.to(dev), **kw)
        ref = ref + R.double()
    e = rel_l2(out, ref)
    print(f"[mxfp8 dx] {epi} tail={tail} {M}x{N}x{K} {gfmt}: rel-L2 {e:.3e}")
    assert e < 5e-3


@pytest.mark.parametrize("ofmt", FMTS)
@pytest.mark.parametrize("gfmt", FMTS)
def test_gemm_mxfp8_dx_fp8_output_copy_exact(dev, gfmt, ofmt):
    """the dGELU product's fp8 copy (d(u) for the fc1 / linear1 product that follows): the bytes must be the clamped CPU cast of the bf16
    output as written over the scale, in either format, the amax slot max |out| exactly; some values saturate"""
    from vt355 import ops
    from vt355.ops import EPI_DGELU
    gen = torch.Generator().manual_seed(3)
    M, N, K = 333, 512, 256
    gq, sg, _ = _quant_g(torch.randn(M, K, generator=gen), gfmt, dev)
    wq, sw, _ = _quant_w(torch.randn(N, K, generator=gen) * K ** -0.5, dev)
    u = torch.randn(M, N, generator=gen).to(BF).to(dev)
    out = poisoned((M, N), BF, dev)
    cq = poisoned((M, N), ofmt, dev)
    sq = torch.tensor([2.0 / FMAX[ofmt]], device=dev)                    # |out| above 2 saturates
    amax = torch.zeros(1, device=dev)
    ops.gemm_mxfp8_dx(gq, wq, out, sg, sw, epilogue=EPI_DGELU, pre_act_in=u, out_fp8=(cq, sq, amax))
    all_written(cq, "fp8 output copy", expect=_fp8_cpu(out, sq, ofmt).to(dev))
    assert torch.equal(_bytes(cq), _bytes(_fp8_cpu(out, sq, ofmt)))
    assert amax.item() == out.float().abs().max().item()
    assert (out.float().abs() > 2.0).any()
    assert bool(torch.isfinite(cq.float()).all()) and cq.float().abs().max().item() == FMAX[ofmt]
    plain = poisoned((M, N), BF, dev)
    ops.gemm_mxfp8_dx(gq, wq, plain, sg, sw, epilogue=EPI_DGELU, pre_act_in=u)
    assert torch.equal(plain, out)                                       # the copy does not change the bf16 output


@pytest.mark.parametrize("fmt", FMTS)
def test_gate_mul_fp8_exact(dev, fmt):
    """vt_gate_mul_fp8: the bf16 output is vt_gate_mul's bit for bit; the fp8 copy is the clamped CPU cast of it, byte for byte; the amax
    exact; some values saturate.  Written into column slices of wider buffers (row strides), whose other columns stay untouched"""
    from vt355 import ops
    gen = torch.Generator().manual_seed(4)
    B, L, D = 2, 75, 384
    M = B * L
    x = (torch.randn(M, D, generator=gen) * 2).to(BF).to(dev)
    gate = torch.randn(B, 3 * D, generator=gen).to(dev)
    g = gate[:, D:2 * D]
    y0 = poisoned((M, D), BF, dev)
    ops.gate_mul(x, y0, g, g, 3 * D, D, L, 0)
    y1 = torch.full((M, D + 64), 5.0, dtype=BF, device=dev)
    q = torch.zeros(M, D + 128, dtype=fmt, device=dev)
    scale = torch.tensor([3.0 / FMAX[fmt]], device=dev)
    amax = torch.zeros(1, device=dev)
    ops.gate_mul_fp8(x, y1[:, :D], g, g, 3 * D, D, L, 0, q[:, 128:], scale, amax)
    assert torch.equal(y1[:, :D], y0) and bool((y1[:, D:] == 5.0).all())
    assert torch.equal(_bytes(q[:, 128:]), _bytes(_fp8_cpu(y0, scale, fmt))) and bool((_bytes(q[:, :128]) == 0).all())
    assert amax.item() == y0.float().abs().max().item()
    assert (y0.float().abs() > 3.0).any() and bool(torch.isfinite(q.float()).all())


@pytest.mark.parametrize("fmt", FMTS)
def test_cast_fp8_fmt_exact(dev, fmt):
    """vt_cast_fp8_fmt: vt_cast_fp8_scaled's semantics in either format -- bytes vs the clamped CPU cast (saturating, never inf), the amax
    accumulated over calls, the row map with its bf16 copy; in E4M3 the bytes are vt_cast_fp8_scaled's"""
    from vt355 import ops
    gen = torch.Generator().manual_seed(5)
    B, Lj, L, off, K = 3, 50, 17, 29, 384
    x = (torch.randn(B * Lj, K, generator=gen) * 3).to(BF).to(dev)
    x[7, 5] = 1e6                                                        # far above FMAX * scale in both formats
    scale = torch.tensor([2.5 / FMAX[fmt]], device=dev)
    y = poisoned((B * Lj, K), fmt, dev)
    amax = torch.zeros(1, device=dev)
    ops.cast_fp8_fmt(x, y, scale, amax)
    all_written(y, "fp8 cast", expect=_fp8_cpu(x, scale, fmt).to(dev))
    assert torch.equal(_bytes(y), _bytes(_fp8_cpu(x, scale, fmt)))
    assert bool(torch.isfinite(y.float()).all()) and y.float()[7, 5].item() == FMAX[fmt]
    assert amax.item() == x.float().abs().max().item()
    assert (x.float().abs() > 2.5).sum().item() > 100
    y2 = poisoned((B * L, K), fmt, dev)
    cp = torch.full((B * L, K + 64), 5.0, dtype=BF, device=dev)
    amax2 = torch.zeros(1, device=dev)
    ops.cast_fp8_fmt(x, y2, scale, amax2, copy=cp[:, :K], rows=(L, Lj, off))
    rows = x.view(B, Lj, K)[:, off:off + L].reshape(B * L, K)
    assert torch.equal(cp[:, :K], rows) and bool((cp[:, K:] == 5.0).all())
    all_written(y2, "fp8 cast through the row map", expect=_fp8_cpu(rows, scale, fmt).to(dev))
    assert torch.equal(_bytes(y2), _bytes(_fp8_cpu(rows, scale, fmt)))
    assert amax2.item() == rows.float().abs().max().item()
    if fmt == E4:
        y3 = poisoned((B * Lj, K), E4, dev)
        ops.cast_fp8_scaled(x, y3, scale, torch.zeros(1, device=dev))
        assert torch.equal(_bytes(y3), _bytes(y))


@pytest.mark.parametrize("fmax", [57344.0, 448.0])
def test_fp8_scale_update_fmax_matches_restatement(dev, fmax):
    """test_fp8_scale_update_matches_restatement's protocol with the divisor as an argument: 20 sites, 20 updates of synthetic amaxes (one
    site always 0, one with a single spike that must leave the window after H updates): rolling window (newest first), max / FMAX (IEEE
    division, on the CPU), 1 for an all-zero history, slots cleared.  With 448 the scales are vt_fp8_scale_update's"""
    from vt355 import ops
    gen = torch.Generator().manual_seed(6)
    n, H, T = 20, 16, 20
    seq = torch.rand(T, n, generator=gen) * torch.logspace(-3, 3, n)
    seq[:, 3] = 0.0
    seq[:, 5] = 0.01; seq[1, 5] = 50.0
    amax = torch.zeros(n, device=dev); hist = torch.zeros(n, H, device=dev); scale = torch.zeros(n, device=dev)
    amax0 = torch.zeros(n, device=dev); hist0 = torch.zeros(n, H, device=dev); scale0 = torch.zeros(n, device=dev)
    h_ref = torch.zeros(n, H)
    for t in range(T):
        amax.copy_(seq[t])
        ops.fp8_scale_update_fmax(amax, hist, scale, fmax)
        h_ref = torch.cat([seq[t][:, None], h_ref[:, :-1]], 1)
        mx = h_ref.max(1).values
        s_ref = torch.where(mx > 0, mx / fmax, torch.ones_like(mx))
        assert torch.equal(hist.cpu(), h_ref) and torch.equal(scale.cpu(), s_ref) and bool((amax == 0).all())
        if fmax == 448.0:
            amax0.copy_(seq[t])
            ops.fp8_scale_update(amax0, hist0, scale0)
            assert torch.equal(scale0, scale) and torch.equal(hist0, hist)
    assert scale[3].item() == 1.0 and scale[5].item() == torch.tensor(0.01) / fmax


# ---- the mode in the model ----
def _rope_tables(S, gen):
    ang = torch.rand(S, 64, generator=gen) * 6.28
    return torch.repeat_interleave(ang.cos(), 2, dim=1).contiguous(), torch.repeat_interleave(ang.sin(), 2, dim=1).contiguous()


def _blocks_inputs(dev, seed):
    """the inputs of test_hunyuan_mxfp8_gpu's model tests"""
    gen = torch.Generator().manual_seed(seed)
    B, Li, Lt, D = 2, 160, 32, 256
    img, txt, vec = torch.randn(B, Li, D, generator=gen).to(BF), torch.randn(B, Lt, D, generator=gen).to(BF), torch.randn(B, D, generator=gen).to(BF)
    cos, sin = _rope_tables(Li, gen)
    dout = torch.randn(B, Li + Lt, D, generator=gen).to(BF)
    return [t.to(dev) for t in (img, txt, vec, torch.tensor([32, 19]), cos, sin, dout)]


def _blocks(dev, dgrad, lora=False):
    from vt355.hunyuan import HunyuanBlocks
    kw = dict(lora_rank=4, lora_alpha=2.0) if lora else {}
    m = HunyuanBlocks(hidden_size=256, heads_num=2, mm_double_blocks_depth=2, mm_single_blocks_depth=2, fp8="mfma", fp8_dgrad=dgrad,
                      **kw).to(dev).init_weights(4)
    if lora:
        m.lora.init_weights(5, zero_b=False)
        return m, m.enable_lora_training()
    return m, m.enable_training()


@pytest.mark.parametrize("lora", [False, True], ids=["fullft", "lora"])
def test_forward_bit_equal_to_mfma(dev, lora):
    """fp8_dgrad touches only the backward: the forward output (fresh histories, same seeds) is bit-equal to fp8="mfma" alone -- on the
    first (just-in-time) forward and on the second (delayed scales), with a backward in between"""
    img, txt, vec, tv, cos, sin, dout = _blocks_inputs(dev, 9)
    outs = {}
    for dg in (False, True, "e4m3"):
        m, _ = _blocks(dev, dg, lora)
        o1 = m(img, txt, vec, tv, (cos, sin))
        o1.backward(dout)
        with torch.no_grad():
            o2 = m(img, txt, vec, tv, (cos, sin))
        outs[dg] = (o1.detach().clone(), o2.clone())
    for dg in (True, "e4m3"):
        assert torch.equal(outs[dg][0], outs[False][0]) and torch.equal(outs[dg][1], outs[False][1])


@pytest.mark.parametrize("fmt", ["e5m2", "e4m3"])
def test_gradient_sites_delayed_scaling(dev, fmt):
    """the forward test's protocol on the gradient state (2 + 2 blocks: 8 * 2 + 3 * 2 = 22 sites).  Backward 1 scales just in time and seeds
    every site (history[:, 0] > 0, scale = history[:, 0] / FMAX); backward 2 with dout x 8 runs on those scales and records larger
    amaxes; backward 3's history holds them and its scales are max(history) / FMAX; every gradient stays finite"""
    fmax = 57344.0 if fmt == "e5m2" else 448.0
    img, txt, vec, tv, cos, sin, dout = _blocks_inputs(dev, 9)
    m, ts = _blocks(dev, fmt)
    assert m.n_fp8_grad_sites == 22
    m(img, txt, vec, tv, (cos, sin)).backward(dout)
    st = m._fp8_grad_state
    assert st.seeded and st.history.shape == (22, 16)
    a1 = st.history[:, 0].clone()
    assert bool((a1 > 0).all()) and torch.equal(st.scale.cpu(), a1.cpu() / fmax)
    m(img, txt, vec, tv, (cos, sin)).backward(dout * 8)
    a2 = st.amax.clone()                                      # recorded by backward 2, rolled in by backward 3
    assert bool((a2 > 0).all()) and bool((a2 > a1).all())
    assert torch.isfinite(ts.grad).all()
    m(img, txt, vec, tv, (cos, sin)).backward(dout)
    h = st.history.cpu()
    assert torch.equal(h[:, 0], a2.cpu()) and torch.equal(h[:, 1], a1.cpu()) and torch.equal(h[:, 2], a1.cpu())
    assert torch.equal(st.scale.cpu(), h.max(1).values / fmax) and torch.equal(st.scale.cpu(), a2.cpu() / fmax)
    assert torch.isfinite(ts.grad).all()


# rel-L2 caps of test_gradients_vs_mfma: twice the worst measured value per format and training mode (the measured values are in its docstring)
_CAPS = {("fullft", "e5m2"): 2 * 6.56e-2, ("fullft", "e4m3"): 2 * 3.30e-2, ("lora", "e5m2"): 2 * 6.69e-2, ("lora", "e4m3"): 2 * 4.10e-2}
# E5M2 tensors measured below the 0.98 cosine aim, by name: (measured cosine, cap = measured - (1 - measured) / 2).  None was: the worst
# measured E5M2 cosine is 0.99783, so 0.98 holds for both formats.
_E5M2_BELOW_AIM = {}


def _grads(dev, dgrad, lora):
    img, txt, vec, tv, cos, sin, dout = _blocks_inputs(dev, 9)
    img = img.clone().requires_grad_(True); txt = txt.clone().requires_grad_(True)
    m, ts = _blocks(dev, dgrad, lora)
    out = m(img, txt, vec, tv, (cos, sin))
    out.backward(dout)
    owner = m.lora if lora else m
    g = {n: owner._view(ts.grad, n).detach().clone() for n in owner.shapes}
    g["d(img)"], g["d(txt)"] = img.grad.detach().clone(), txt.grad.detach().clone()
    return g


@pytest.mark.parametrize("lora", [False, True], ids=["fullft", "lora"])
def test_gradients_vs_mfma(dev, lora):
    """every parameter gradient (full fine-tune: all Linear weights and biases, the modulation Linears and the q / k norm weights; LoRA
    rank 4, zero_b=False: every adapter) and d(img), d(txt), against fp8="mfma" alone -- the parent's bf16 backward, never the mode
    itself.  No tensor is left out.
    Fixed in advance: for "e4m3" every tensor's cosine to "mfma" mode is > 0.98 (the project's gradient tolerance); for "e5m2"
    0.98 is the aim and a tensor below it is listed by name in _E5M2_BELOW_AIM with its measured value, its cap being that value minus half
    its distance to 1; over all tensors together "e4m3" is closer to "mfma" mode than "e5m2" in rel-L2.  The rel-L2 caps are twice the
    worst measured per-tensor value (margin for other draws; dQ's summation order moves the figures by ~1e-6 between runs).
    Measured (MI355X), worst per-tensor rel-L2 / worst cosine / all tensors together:
      full fine-tune, 66 tensors: e4m3 3.30e-2 (double_blocks.0.txt_attn_q_norm.weight) / 0.99946 / 1.54e-2;
                                  e5m2 6.56e-2 (double_blocks.0.img_attn_k_norm.weight) / 0.99785 / 2.98e-2; d(img) 1.08e-2 / 1.95e-2
      LoRA, 30 tensors:           e4m3 4.10e-2 (double_blocks.1.img_attn_qkv.lora_A.v.weight) / 0.99923 / 1.23e-2;
                                  e5m2 6.69e-2 (the same tensor) / 0.99783 / 2.21e-2; d(img) 1.96e-2 (e5m2)
    -- below the unattenuated quadrature estimate (9 % / 18 %): the un-quantised residual path dilutes the roundings."""
    key = "lora" if lora else "fullft"
    ref = _grads(dev, False, lora)
    tot, res = {}, {}
    for fmt in ("e4m3", "e5m2"):                       # measure and print everything before the first assertion
        got = _grads(dev, fmt, lora)
        assert set(got) == set(ref)
        rows = sorted(((rel_l2(got[n], ref[n]), cosine(got[n], ref[n]), n) for n in ref), reverse=True)
        num = sum((got[n].double() - ref[n].double()).pow(2).sum().item() for n in ref)
        den = sum(ref[n].double().pow(2).sum().item() for n in ref)
        tot[fmt] = (num / den) ** 0.5
        worst_cos = min(rows, key=lambda r: r[1])
        below = {n: c for a, c, n in rows if c <= 0.98}
        res[fmt] = (got, rows, below)
        print(f"[hunyuan dgrad {key} {fmt}] {len(rows)} tensors; worst rel-L2 {rows[0][0]:.4e} ({rows[0][2]}); worst cosine {worst_cos[1]:.5f} "
              f"({worst_cos[2]}); all tensors together rel-L2 {tot[fmt]:.4e}; five worst: {[(n, f'{a:.3e}', f'{c:.5f}') for a, c, n in rows[:5]]}; "
              f"d(img) {[f'{a:.3e}' for a, c, n in rows if n == 'd(img)']} d(txt) {[f'{a:.3e}' for a, c, n in rows if n == 'd(txt)']}; "
              f"tensors below the 0.98 cosine aim: {below}")
    for fmt in ("e4m3", "e5m2"):
        got, rows, below = res[fmt]
        assert all(torch.isfinite(got[n].float()).all() for n in got)
        assert not any(torch.equal(got[n], ref[n]) for n in ("d(img)", "d(txt)"))      # the fp8 products ran
        if fmt == "e4m3":
            assert not below, below
        else:
            for n, c in below.items():
                assert n in _E5M2_BELOW_AIM and c > _E5M2_BELOW_AIM[n][1], (n, c)
        cap = _CAPS[(key, fmt)]
        assert cap is not None and rows[0][0] < cap, (rows[0], cap)
    assert tot["e4m3"] < tot["e5m2"]


def test_whole_model_training_steps_dgrad(dev):
    """HYVideoDiffusionTransformer (2 + 2 blocks, LoRA r 4, fp8="mfma") through HunyuanVideoFlow.training_step for 5 optimizer steps on the
    fixed batches and draws of test_whole_model_training_steps, gradients in E5M2 and in E4M3: every loss finite and within 2e-2 relative
    of the bf16 run's (that test's bar).  Measured worst (MI355X): 3.5e-4 (e5m2), 3.3e-4 (e4m3)"""
    from vt355.hunyuan import HYVideoDiffusionTransformer, HunyuanVideoFlow
    gen = torch.Generator().manual_seed(21)
    B, Lt = 2, 24
    mask = (torch.arange(Lt)[None, :] < torch.tensor([24, 13])[:, None]).long()
    batches = [{"latents": torch.randn(B, 4, 3, 8, 12, generator=gen), "prompt_embeds": torch.randn(B, Lt, 64, generator=gen).to(BF),
                "prompt_attention_mask": mask, "pooled_prompt_embeds": torch.randn(B, 32, generator=gen).to(BF)} for _ in range(5)]
    losses = {}
    for mode, dg in ((False, False), ("mfma", "e5m2"), ("mfma", "e4m3")):
        m = HYVideoDiffusionTransformer(in_channels=4, hidden_size=256, heads_num=2, mm_double_blocks_depth=2, mm_single_blocks_depth=2,
                                        text_states_dim=64, text_states_dim_2=32, lora_rank=4, fp8=mode, fp8_dgrad=dg).to(dev).init_weights(11)
        m.lora.init_weights(12, zero_b=False)
        flow = HunyuanVideoFlow(model=m, learning_rate=1e-4).to(dev)
        opt = flow.configure_optimizers()
        ls = []
        for i, b in enumerate(batches):
            torch.manual_seed(100 + i)
            loss = flow.training_step({k: v.to(dev) for k, v in b.items()})
            loss.backward()
            opt.step()
            opt.zero_grad()
            ls.append(loss.item())
        losses[dg] = ls
        if dg:
            assert m._fp8_grad_state.seeded and bool((m._fp8_grad_state.history[:, 0] > 0).all())
    for dg in ("e5m2", "e4m3"):
        rel = [abs(a - b) / abs(b) for a, b in zip(losses[dg], losses[False])]
        print(f"[hunyuan dgrad model {dg}] losses bf16 {losses[False]} dgrad {losses[dg]} worst rel {max(rel):.3e}")
        assert all(torch.isfinite(torch.tensor(v)) for v in losses[dg])
        assert max(rel) < 2e-2
