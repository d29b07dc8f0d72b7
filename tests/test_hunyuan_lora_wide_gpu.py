"""HunyuanVideo LoRA ranks 22..128 on the wide K-extension layout: the wide bf16 tail of vt_gemm_mxfp8 / vt_gemm_mxfp8_dx (Kt up to 384,
staged through LDS), then HunyuanBlocks / HYVideoDiffusionTransformer at wide ranks in bf16 and in the fp8 modes, against the fp64 oracle
and against the narrow-rank tests' own bars."""
import os

import numpy as np
import pytest
import torch

from parity import bf16_leaves, cosine, floor_report, poisoned, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
FMAX = {E4: 448.0, E5: 57344.0}
GFMTS = [pytest.param(E5, id="e5m2"), pytest.param(E4, id="e4m3")]
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WIDE_KTS = [96, 128, 192, 384]


# ---------------------------------------------------------------------------------------------------------------- the tail kernel, exact
def _exact_operands(Kt, ones=False, seed=3):
    """M, N, K = 300, 260, 384: fp8 operands in {-2..2} (with `ones`: {-1, 0, 1}), tail operands in {-1, 0, 1} (with `ones`: all 1, so that
    every 32-column step of the tail adds 32 to EVERY result), as fp32 tensors holding integers.  Returns (a, w, at, wt, fp64 result with
    the tail, fp64 result without it); asserts what makes the comparison exact and meaningful: |result| <= 256 (integers up to 256 are
    bf16 numbers, so the one rounding at the store is exact) and, in every 16 x 16 tile, a result that differs without the tail."""
    M, N, K = 300, 260, 384
    gen = torch.Generator().manual_seed(seed)
    lim = 1 if ones else 2
    a = torch.randint(-lim, lim + 1, (M, K), generator=gen).float()
    w = torch.randint(-lim, lim + 1, (N, K), generator=gen).float()
    if ones:
        at, wt = torch.ones(M, Kt), torch.ones(N, Kt)
    else:
        at = torch.randint(-1, 2, (M, Kt), generator=gen).float()
        wt = torch.randint(-1, 2, (N, Kt), generator=gen).float()
    base = a.double() @ w.double().t()
    ref = base + at.double() @ wt.double().t()
    assert ref.abs().max().item() <= 256 and base.abs().max().item() <= 256
    diff = torch.zeros(304, 272, dtype=torch.bool)
    diff[:M, :N] = ref != base
    assert bool(diff.view(19, 16, 17, 16).any(3).any(1).all()), "a tile whose results do not depend on the tail"
    if ones:
        assert bool((ref != base).all())
    return a, w, at, wt, ref, base


def _sliced(t, dev, left, right, fill=5.0):
    """t as a column slice [:, left : left + Kt] of a wider bf16 device buffer whose other columns hold `fill` (a value that would change
    the result if the kernel read it as part of the tail); left % 8 == 0 keeps the slice 16-byte aligned"""
    buf = torch.full((t.shape[0], left + t.shape[1] + right), fill, dtype=BF, device=dev)
    buf[:, left:left + t.shape[1]] = t.to(dev, BF)
    v = buf[:, left:left + t.shape[1]]
    assert v.stride(0) > t.shape[1] and v.data_ptr() % 16 == 0
    return v


@pytest.mark.parametrize("Kt,ones", [(kt, False) for kt in WIDE_KTS] + [(192, True)])
def test_gemm_mxfp8_wide_tail_exact(dev, Kt, ones):
    """small integers: the fp8 sum, its scaling by 1 * 1 and the bf16 tail's products are exact in fp32 and the result a bf16 number, so the
    output must equal the integer result bit for bit; the tail operands are column slices of wider buffers (ld > Kt) with ragged M and N
    (edge tiles).  Kt = 96: a last step of 32 columns.  `ones`: every step of the tail moves every element"""
    from vt355 import ops
    a, w, at, wt, ref, base = _exact_operands(Kt, ones)
    one = torch.ones(1, device=dev)
    out = poisoned((300, 260), BF, dev)
    ops.gemm_mxfp8(a.to(E4).to(dev), w.to(E4).to(dev), out, one, one, tail=(_sliced(at, dev, 256, 40), _sliced(wt, dev, 384, 8)))
    assert torch.equal(out.cpu(), ref.to(BF))
    assert not torch.equal(out.cpu(), base.to(BF))


@pytest.mark.parametrize("gfmt", GFMTS)
@pytest.mark.parametrize("Kt,ones", [(kt, False) for kt in WIDE_KTS] + [(192, True)])
def test_gemm_mxfp8_dx_wide_tail_exact(dev, Kt, ones, gfmt):
    """the same through vt_gemm_mxfp8_dx, the gradient operand in E5M2 and in E4M3 (the integers are exact in both)"""
    from vt355 import ops
    a, w, at, wt, ref, base = _exact_operands(Kt, ones)
    assert torch.equal(a.to(gfmt).float(), a)
    one = torch.ones(1, device=dev)
    out = poisoned((300, 260), BF, dev)
    ops.gemm_mxfp8_dx(a.to(gfmt).to(dev), w.to(E4).to(dev), out, one, one, tail=(_sliced(at, dev, 256, 40), _sliced(wt, dev, 384, 8)))
    assert torch.equal(out.cpu(), ref.to(BF))
    assert not torch.equal(out.cpu(), base.to(BF))


# ---------------------------------------------------------------------------------------------------------------- the tail kernel, random
def _gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def _gelu_tanh_grad(x):
    c = 0.7978845608028654
    t = torch.tanh(c * (x + 0.044715 * x ** 3))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * c * (1.0 + 3.0 * 0.044715 * x * x)


def _quant(x, dev):
    from vt355 import ops
    xq, s = ops.quantize_fp8(x.to(dev, BF).contiguous())
    return xq, s, xq.double().cpu() * s.double().cpu()


def _quant_g(x, dt, dev):
    xb = x.to(BF)
    s = (xb.float().abs().max() / FMAX[dt]).reshape(1)
    q = (xb.float() / s).clamp(-FMAX[dt], FMAX[dt]).to(dt)
    return q.to(dev), s.to(dev), q.double() * s.double()


@pytest.mark.parametrize("Kt", [192, 384])
@pytest.mark.parametrize("epi", ["bias", "gelu", "gated"])
def test_gemm_mxfp8_wide_tail_random_vs_fp64(dev, epi, Kt):
    """test_gemm_mxfp8_random_vs_fp64's small shape and bar (5e-3) with a 192- / 384-column tail, every epilogue: the tail adds bf16
    products that are exact in fp32, so the bf16 rounding of the output is still all that is left"""
    from vt355 import ops
    from vt355.ops import EPI_BIAS_GELU, EPI_GATED_RES
    M, N, K = 200, 384, 256
    gen = torch.Generator().manual_seed(2)
    aq, sa, ad = _quant(torch.randn(M, K, generator=gen), dev)
    wq, sw, wd = _quant(torch.randn(N, K, generator=gen) * K ** -0.5, dev)
    bias = (torch.randn(N, generator=gen) * 0.1).to(BF)
    At = (torch.randn(M, Kt, generator=gen) * 0.5).to(BF); Wt = (torch.randn(N, Kt, generator=gen) * 0.1).to(BF)
    ref = ad @ wd.t() + bias.double() + At.double() @ Wt.double().t()
    kw = dict(tail=(_sliced(At, dev, 256, 0), _sliced(Wt, dev, 256, 0)))
    out = poisoned((M, N), BF, dev)
    if epi == "bias":
        ops.gemm_mxfp8(aq, wq, out, sa, sw, bias.to(dev), **kw)
        errs = [rel_l2(out, ref)]
    elif epi == "gelu":
        u = poisoned((M, N), BF, dev)
        ops.gemm_mxfp8(aq, wq, out, sa, sw, bias.to(dev), epilogue=EPI_BIAS_GELU, pre_act_out=u, **kw)
        errs = [rel_l2(u, ref), rel_l2(out, _gelu_tanh(ref))]
    else:
        S = M // 2
        R = torch.randn(M, N, generator=gen).to(BF)
        gate = torch.randn(2, 3 * N, generator=gen)
        branch = poisoned((M, N), BF, dev)
        gd = gate.to(dev)[:, :N]
        ops.gemm_mxfp8(aq, wq, out, sa, sw, bias.to(dev), epilogue=EPI_GATED_RES, residual=R.to(dev), gate_txt=gd, gate_vid=gd,
                       gate_bstride=3 * N, S=S, St=0, pre_act_out=branch, **kw)
        g = gate[:, :N].double()[(torch.arange(M) // S).clamp_max(1)]
        errs = [rel_l2(branch, ref), rel_l2(out, R.double() + g * ref)]
    print(f"[mxfp8 wide tail] {epi} Kt={Kt}: rel-L2 {[f'{e:.3e}' for e in errs]}")
    assert all(e < 5e-3 for e in errs)


@pytest.mark.parametrize("gfmt", GFMTS)
@pytest.mark.parametrize("Kt", [192, 384])
@pytest.mark.parametrize("epi", ["plain", "dgelu", "res"])
def test_gemm_mxfp8_dx_wide_tail_random_vs_fp64(dev, epi, Kt, gfmt):
    """test_gemm_mxfp8_dx_random_vs_fp64's small shape and bar (5e-3) with a 192- / 384-column tail, every epilogue, both formats"""
    from vt355 import ops
    from vt355.ops import EPI_DGELU, EPI_GATED_RES
    M, N, K = 200, 384, 256
    gen = torch.Generator().manual_seed(2)
    gq, sg, gd = _quant_g(torch.randn(M, K, generator=gen), gfmt, dev)
    wq, sw, wd = _quant(torch.randn(N, K, generator=gen) * K ** -0.5, dev)
    At = (torch.randn(M, Kt, generator=gen) * 0.5).to(BF); Wt = (torch.randn(N, Kt, generator=gen) * 0.1).to(BF)
    ref = gd @ wd.t() + At.double() @ Wt.double().t()
    kw = dict(tail=(_sliced(At, dev, 256, 0), _sliced(Wt, dev, 256, 0)))
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
    print(f"[mxfp8 dx wide tail] {epi} Kt={Kt} {gfmt}: rel-L2 {e:.3e}")
    assert e < 5e-3


# ---------------------------------------------------------------------------------------------------------------- blocks vs the oracle
def _golden():
    g = np.load(os.path.join(G, "hunyuan_blocks.npz"))
    return lambda k: torch.from_numpy(g[k])


def _b(t):
    return t.detach().to(BF).requires_grad_(True)


def _lora_effective(base, ad, sites, s, D):
    """W + scaling * B A on the rows of each adapted projection, in the dtype of base / ad"""
    Pe = dict(base)
    for mod, tags in sites.items():
        w = base[mod + ".weight"].clone()
        for j, t in enumerate(tags):
            dot = "." + t if t else ""
            w[j * D:(j + 1) * D] = w[j * D:(j + 1) * D] + s * ad[f"{mod}.lora_B{dot}.weight"] @ ad[f"{mod}.lora_A{dot}.weight"]
        Pe[mod + ".weight"] = w
    return Pe


def _golden_blocks(dev, r, seed=5):
    """test_lora_blocks_train_step_matches_oracle's model: D 256, 2 heads, one double + one single block, the oracle's weights,
    adapters with zero_b=False"""
    import hunyuan_oracle as HO
    from vt355.hunyuan import HunyuanBlocks
    D, H = 256, 2
    m = HunyuanBlocks(hidden_size=D, heads_num=H, mm_double_blocks_depth=1, mm_single_blocks_depth=1, lora_rank=r, lora_alpha=2.0)
    P = {**HO.init(HO.double_block_shapes(D, H, pre="double_blocks.0."), 1), **HO.init(HO.single_block_shapes(D, H, pre="single_blocks.0."), 2)}
    m.load_state_dict(P, strict=False)
    m.lora.init_weights(seed, zero_b=False)
    m.to(dev)
    return HO, m


@pytest.mark.parametrize("r,knob", [(22, False), (24, False), (64, False), (128, False), (4, True)],
                         ids=["r22", "r24", "r64", "r128", "r4-VT355_LORA_WIDE"])
def test_wide_lora_blocks_train_step_matches_oracle(dev, monkeypatch, r, knob):
    """test_lora_blocks_train_step_matches_oracle at the wide ranks (22: the first one, ragged padding; 24: r % 16 != 0; 64: a 192-column
    extension; 128: the maximum) and at rank 4 under VT355_LORA_WIDE=1: forward, input gradients and every adapter gradient against the
    fp64 oracle on the effective weights W + scaling B A, with that test's bars (forward 1e-2, input gradients 3e-2, adapter gradients
    under parity.floor_bars at cosine 0.98 / cap 0.2; no parameter has a margin of its own)"""
    if knob:
        monkeypatch.setenv("VT355_LORA_WIDE", "1")
    else:
        monkeypatch.delenv("VT355_LORA_WIDE", raising=False)
    T = _golden()
    D, H = 256, 2
    HO, m = _golden_blocks(dev, r)
    assert m.lora.wide and m.lora.rp == (r + 15) // 16 * 16
    ts = m.enable_lora_training()
    assert m.train_state is None and ts.numel == m.lora.numel
    tv = T("txt_valid")
    img, txt, vec = [T(k).to(BF) for k in ("img", "txt", "vec")]
    Lt = txt.shape[1]
    xi, xt, xv = [t.to(dev).requires_grad_(True) for t in (img, txt, vec)]
    out = m(xi, xt, xv, tv.to(dev), (T("cos").to(dev), T("sin").to(dev)))
    gx = T("s_gx").to(BF)
    out.backward(gx.to(dev))
    base = {k: v.detach().float().cpu().double() for k, v in m.named_parameters() if not k.startswith("lora.")}
    ad = {k[5:]: v.detach().float().cpu().double().requires_grad_(True) for k, v in m.named_parameters() if k.startswith("lora.")}
    Pe = _lora_effective(base, ad, m.lora.sites, m.lora.scaling, D)
    ri, rt, rv = [t.double().requires_grad_(True) for t in (img, txt, vec)]
    io, to = HO.double_block(ri, rt, rv, Pe, "double_blocks.0.", H, tv, T("cos").double(), T("sin").double())
    xo = HO.single_block(torch.cat([io, to], 1), rv, Pe, "single_blocks.0.", H, Lt, tv, T("cos").double(), T("sin").double())
    (xo * gx.double()).sum().backward()
    vm = (gx.abs().sum(-1, keepdim=True) > 0).double()
    tm = (T("d_gt").abs().sum(-1, keepdim=True) > 0)
    e = rel_l2(out.double().cpu() * vm, xo * vm)
    ei, et = rel_l2(xi.grad, ri.grad), rel_l2(xt.grad.double().cpu() * tm, rt.grad * tm)
    adb = bf16_leaves(ad)
    Pb = _lora_effective({k: v.detach().to(BF) for k, v in base.items()}, adb, m.lora.sites, m.lora.scaling, D)
    bi, bt = HO.double_block(_b(img), _b(txt), _b(vec), Pb, "double_blocks.0.", H, tv, T("cos"), T("sin"))
    bo = HO.single_block(torch.cat([bi, bt], 1), _b(vec), Pb, "single_blocks.0.", H, Lt, tv, T("cos"), T("sin"))
    assert bo.dtype == BF
    (bo.float() * gx.float()).sum().backward()
    overall, ofloor, worst, bad, ratio, at = floor_report([(n, m.lora._view(ts.grad, n), ad[n].grad) for n in m.lora.shapes],
                                                          {n: adb[n].grad for n in m.lora.shapes}, 0.98, 0.2)
    print(f"[hunyuan lora wide r{r}] fwd rel-L2 {e:.3e}, d(img) {ei:.3e}, d(txt) {et:.3e}; adapter grads overall rel-L2 {overall:.3e} "
          f"(bf16 floor {ofloor:.3e}), worst {worst:.3e}, worst device / floor {ratio:.2f} at {at}")
    assert e < 1e-2
    assert ei < 3e-2 and et < 3e-2
    assert not bad, bad[:8]
    assert overall < 1.5 * ofloor, (overall, ofloor)


def _random_inputs(dev, seed, B=2, Li=160, Lt=32, D=256):
    gen = torch.Generator().manual_seed(seed)
    img, txt, vec = torch.randn(B, Li, D, generator=gen).to(BF), torch.randn(B, Lt, D, generator=gen).to(BF), torch.randn(B, D, generator=gen).to(BF)
    ang = torch.rand(Li, 64, generator=gen) * 6.28
    cos, sin = torch.repeat_interleave(ang.cos(), 2, dim=1).contiguous(), torch.repeat_interleave(ang.sin(), 2, dim=1).contiguous()
    dout = torch.randn(B, Li + Lt, D, generator=gen).to(BF)
    return [t.to(dev) for t in (img, txt, vec, torch.tensor([32, 19][:B]), cos, sin, dout)]


@pytest.mark.parametrize("r", [24, 128])
def test_repack_after_a_step_is_a_fresh_pack(dev, monkeypatch, r):
    """after FusedAdamW.step() the extension columns / rows are rewritten by vt_lora_pack_b(t)_wide while the base columns stay: a freshly
    built model loaded from the stepped state dict (packed from scratch) must give the same forward bit for bit"""
    from vt355.hunyuan import HunyuanBlocks
    from vt355.optim import FusedAdamW
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False)
    img, txt, vec, tv, cos, sin, dout = _random_inputs(dev, 21, B=1, Li=40, Lt=8)
    _, m = _golden_blocks(dev, r)
    ts = m.enable_lora_training()
    out = m(img, txt, vec, tv, (cos, sin))
    out.backward(dout)
    opt = FusedAdamW(ts.params, lr=1e-3, fullft_state=ts)
    before = ts.flat.clone()
    opt.step()
    assert torch.isfinite(ts.flat).all() and (ts.flat - before).abs().max().item() > 0
    with torch.no_grad():
        out2 = m(img, txt, vec, tv, (cos, sin))
    assert not torch.equal(out2, out.detach())                    # the repacked adapters are used
    m2 = HunyuanBlocks(hidden_size=256, heads_num=2, mm_double_blocks_depth=1, mm_single_blocks_depth=1, lora_rank=r, lora_alpha=2.0)
    m2.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
    m2.to(dev)
    with torch.no_grad():
        out3 = m2(img, txt, vec, tv, (cos, sin))
    assert torch.isfinite(out3.float()).all() and torch.equal(out3, out2)


def test_partial_backward_touches_only_the_adapters_it_reaches(dev, monkeypatch):
    """a backward that stops at the single block's input: the single block's adapters get the gradients of the full run (the same launches;
    the fp32 atomics of vt_lora_tn_wide leave them equal to rounding, 1e-4 here, far inside the oracle bars), the double block's adapters
    -- whose Linears the backward never reached -- stay exactly zero.  Nothing is staged, so nothing depends on how many sites ran."""
    from vt355.hunyuan import _HYRun
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False)
    img, txt, vec, tv, cos, sin, dout = _random_inputs(dev, 22, B=1, Li=40, Lt=8)
    grads = {}
    for part in (False, True):
        _, m = _golden_blocks(dev, 24)
        ts = m.enable_lora_training()
        run = _HYRun(m, save=True)
        marks = []
        single = run.single_block
        run.single_block = lambda *a, **k: (marks.append(len(run.tape)), single(*a, **k))[1]
        out = run.forward(img, txt, vec, tv, (cos, sin))
        assert len(marks) == 1 and 0 < marks[0] < len(run.tape)
        if part:
            run._out.g = dout.reshape(-1, 256).contiguous()
            while len(run.tape) > marks[0]:
                run.tape.pop()()
        else:
            run.backward(dout)
        grads[part] = {n: m.lora._view(ts.grad, n).detach().clone() for n in m.lora.shapes}
    touched = [n for n in grads[True] if n.startswith("single_blocks.")]
    untouched = [n for n in grads[True] if not n.startswith("single_blocks.")]
    assert len(touched) == 6 and len(untouched) == 8
    for n in touched:
        assert grads[False][n].abs().max().item() > 0
        assert rel_l2(grads[True][n], grads[False][n]) < 1e-4 and cosine(grads[True][n], grads[False][n]) > 0.98, n
    for n in untouched:
        assert grads[False][n].abs().max().item() > 0 and not bool(grads[True][n].any()), n


# ---------------------------------------------------------------------------------------------------------------- the fp8 modes
def _fp8_blocks(dev, mode, dgrad=False, r=64):
    """test_blocks_lora_tail's model at rank r: 2 + 2 blocks, frozen weights, adapters with zero_b=False and B x 10"""
    from vt355.hunyuan import HunyuanBlocks
    m = HunyuanBlocks(hidden_size=256, heads_num=2, mm_double_blocks_depth=2, mm_single_blocks_depth=2, fp8=mode, fp8_dgrad=dgrad, lora_rank=r,
                      lora_alpha=2.0).to(dev).init_weights(4)
    m.lora.init_weights(5, zero_b=False)
    with torch.no_grad():
        for n, p in m.lora._plist.items():
            if ".lora_B" in n:
                p.mul_(10.0)
    return m, m.enable_lora_training()


# test_gradients_vs_mfma's rel-L2 caps of its LoRA case (tests/test_hunyuan_fp8_dgrad_gpu.py: _CAPS), cosine > 0.98 for every tensor
_DGRAD_CAPS = {"e5m2": 2 * 6.69e-2, "e4m3": 2 * 4.10e-2}


def test_fp8_mfma_and_dgrad_at_rank_64(dev, monkeypatch):
    """rank 64 (a 192-column tail in the forward products and in the fp8 dX products): the forward is bit-equal with fp8_dgrad on and off
    (first, just-in-time forward and second, delayed-scale forward); with fp8_dgrad every adapter gradient and d(img), d(txt) stay within
    test_gradients_vs_mfma's LoRA bars of the fp8="mfma"-alone model (its bf16 backward), and the fp8 products did run"""
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False)
    img, txt, vec, tv, cos, sin, dout = _random_inputs(dev, 11)
    outs, grads = {}, {}
    for dg in (False, "e5m2", "e4m3"):
        m, ts = _fp8_blocks(dev, "mfma", dg)
        assert m.lora.ext_qkv == 192
        xi, xt = img.clone().requires_grad_(True), txt.clone().requires_grad_(True)
        o1 = m(xi, xt, vec, tv, (cos, sin))
        o1.backward(dout)
        with torch.no_grad():
            o2 = m(img, txt, vec, tv, (cos, sin))
        outs[dg] = (o1.detach().clone(), o2.clone())
        g = {n: m.lora._view(ts.grad, n).detach().clone() for n in m.lora.shapes}
        g["d(img)"], g["d(txt)"] = xi.grad.detach().clone(), xt.grad.detach().clone()
        grads[dg] = g
    ref, tot, rows_of = grads[False], {}, {}
    for fmt in ("e4m3", "e5m2"):                               # measure and print everything before the first assertion
        got = grads[fmt]
        rows = sorted(((rel_l2(got[n], ref[n]), cosine(got[n], ref[n]), n) for n in ref), reverse=True)
        num = sum((got[n].double() - ref[n].double()).pow(2).sum().item() for n in ref)
        den = sum(ref[n].double().pow(2).sum().item() for n in ref)
        tot[fmt] = (num / den) ** 0.5
        rows_of[fmt] = rows
        wc = min(rows, key=lambda r_: r_[1])
        print(f"[hunyuan dgrad r64 {fmt}] {len(rows)} tensors; worst rel-L2 {rows[0][0]:.4e} ({rows[0][2]}); worst cosine {wc[1]:.5f} ({wc[2]}); "
              f"all tensors together {tot[fmt]:.4e}")
    for fmt in ("e4m3", "e5m2"):
        assert torch.equal(outs[fmt][0], outs[False][0]) and torch.equal(outs[fmt][1], outs[False][1])
        assert torch.isfinite(outs[fmt][0].float()).all()
        rows = rows_of[fmt]
        assert len(rows) == 2 * 8 + 2 * 6 + 2
        assert not any(torch.equal(grads[fmt][n], ref[n]) for n in ("d(img)", "d(txt)"))           # the fp8 dX products ran
        assert all(c > 0.98 for _, c, _ in rows), [x for x in rows if not x[1] > 0.98]
        assert rows[0][0] < _DGRAD_CAPS[fmt], rows[0]
    assert tot["e4m3"] < tot["e5m2"]


def test_fp8_weights_mode_at_rank_64_is_the_bf16_model_on_dequantised_weights(dev, monkeypatch):
    """fp8="weights" with rank-64 adapters: W_ext's base columns are the de-quantised E4M3 weights, so a bf16 model loaded with those
    (and the same adapters) gives the same output bit for bit"""
    from vt355 import ops
    from vt355.hunyuan import HunyuanBlocks
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False)
    img, txt, vec, tv, cos, sin, _ = _random_inputs(dev, 10, B=1, Li=40, Lt=8)
    kw = dict(hidden_size=256, heads_num=2, mm_double_blocks_depth=1, mm_single_blocks_depth=1, lora_rank=64, lora_alpha=2.0)
    mq = HunyuanBlocks(fp8="weights", **kw).to(dev).init_weights(6)
    mq.lora.init_weights(5, zero_b=False)
    mb = HunyuanBlocks(fp8=False, **kw).to(dev).init_weights(6)
    sd = {}
    for k, v in mq.state_dict().items():
        if k in mq.shapes and k.endswith(".weight") and len(mq.shapes[k]) == 2:
            wq, sw = ops.quantize_fp8(v.to(dev, BF).contiguous())
            v = (wq.float() * sw).to(BF)
        sd[k] = v
    mb.load_state_dict(sd, strict=True)
    with torch.no_grad():
        oq = mq(img, txt, vec, tv, (cos, sin))
        ob = mb(img, txt, vec, tv, (cos, sin))
        for p in mb.lora._plist.values():
            p.zero_()
        mb.lora._packed = None
        o0 = mb(img, txt, vec, tv, (cos, sin))
    assert torch.isfinite(oq.float()).all() and torch.equal(oq, ob)
    assert not torch.equal(o0, ob)                              # the adapters contribute


# ---------------------------------------------------------------------------------------------------------------- the whole model
def test_whole_model_flow_training_step_at_rank_64(dev, monkeypatch):
    """HYVideoDiffusionTransformer(lora_rank=64) at test_hunyuan_gpu's tiny size through HunyuanVideoFlow.training_step, backward and an
    optimizer step: the loss is finite and every adapter moves"""
    import hunyuan_oracle as HO
    from vt355.hunyuan import HunyuanVideoFlow, HYVideoDiffusionTransformer
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False)
    m = HYVideoDiffusionTransformer(in_channels=4, hidden_size=256, heads_num=2, mm_double_blocks_depth=1, mm_single_blocks_depth=1,
                                    text_states_dim=64, text_states_dim_2=32, lora_rank=64, lora_alpha=2.0)
    m.load_state_dict(HO.init_model(HO.model_shapes(256, 2, 1, 1, 4, 4, (1, 2, 2), 64, 32), 3), strict=False)
    m.lora.init_weights(5, zero_b=False)
    m.to(dev)
    flow = HunyuanVideoFlow(model=m, learning_rate=1e-3).to(dev)
    opt = flow.configure_optimizers()
    g = np.load(os.path.join(G, "hunyuan_model.npz"))
    T = lambda k: torch.from_numpy(g[k]).to(dev)
    batch = {"latents": T("x"), "prompt_embeds": T("text_states"), "prompt_attention_mask": T("text_mask"), "pooled_prompt_embeds": T("text_states_2")}
    torch.manual_seed(0)
    before = {n: p.detach().clone() for n, p in m.lora._plist.items()}
    loss = flow.training_step(batch)
    loss.backward()
    ts = m.lora.train_state
    assert torch.isfinite(loss) and torch.isfinite(ts.grad).all()
    opt.step()
    assert torch.isfinite(ts.flat).all()
    still = [n for n, p in m.lora._plist.items() if torch.equal(p.detach(), before[n])]
    assert not still, still
    loss2 = flow.training_step(batch)
    assert torch.isfinite(loss2)


# ---------------------------------------------------------------------------------------------------------------- sequence parallelism
def test_wide_layout_under_ulysses_world2_matches_unsharded(dev, monkeypatch):
    """test_hunyuan_sp_gpu's two-rank LoRA check (2 + 2 blocks, rank 4) with VT355_LORA_WIDE=1, which the spawned ranks inherit: the wide
    layout's adapter gradients are partial sums per rank as the narrow layout's are -- summed over the ranks they equal the unsharded
    run's, under that test's bars"""
    import torch.multiprocessing as mp
    from test_hunyuan_sp_gpu import _free_port, _worker
    monkeypatch.setenv("VT355_LORA_WIDE", "1")
    mgr = mp.Manager(); res = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), True, res), nprocs=2, join=True)
    for r in (0, 1):
        print(f"[hunyuan sp-2 lora wide] rank {r}: " + ", ".join(f"{k} {v:.2e}" for k, v in res[r].items()))
        for k, v in res[r].items():
            assert v < (5e-2 if k == "worst_param" else 1e-2), (r, k, v)
