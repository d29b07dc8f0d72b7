"""HunyuanVideo fp8="mfma": the MX-scaled fp8 GEMM (vt_gemm_mxfp8) and the delayed-scaling kernels that feed it (vt_cast_fp8_scaled,
vt_ln_modulate_fwd_fp8, vt_fp8_scale_update), then the mode in HunyuanBlocks / HYVideoDiffusionTransformer against the bf16 and
fp8="weights" runs of the same weights."""
import pytest
import torch

from parity import all_written, poisoned, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F8 = torch.float8_e4m3fn


def _e4m3_cpu(x_bf16, scale):
    """satfinite(RNE(x / scale)) on the CPU (IEEE division; this torch build's GPU division is not correctly rounded)"""
    return (x_bf16.float().cpu() / scale.float().cpu()).clamp(-448.0, 448.0).to(F8)


def _bytes(t):
    return t.cpu().view(torch.uint8)


def _gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


@pytest.mark.parametrize("M,N,K", [(128, 128, 128), (300, 260, 384)])
def test_gemm_mxfp8_lane_map_exact(dev, M, N, K):
    """small integers are exact in E4M3 and their fp32 sums exact: the result must equal the integer product rounded once to bf16.  A and
    W are independent random integers (W is not symmetric, A != W), so a swapped row / column map or A and B disagreeing on the k order
    inside a 128-deep step cannot pass; ragged M and N exercise the edge tiles; power-of-two scales keep it exact"""
    from vt355 import ops
    gen = torch.Generator().manual_seed(1)
    a = torch.randint(-4, 5, (M, K), generator=gen).float()
    w = torch.randint(-3, 4, (N, K), generator=gen).float()
    w[0, 0], w[1, K - 1] = 7.0, -6.0
    aq, wq = a.to(F8).to(dev), w.to(F8).to(dev)
    sa = torch.tensor([0.5], device=dev); sw = torch.tensor([4.0], device=dev)
    out = torch.full((M, N), 3.0, dtype=BF, device=dev)
    ops.gemm_mxfp8(aq, wq, out, sa, sw)
    ref = ((a.double() @ w.double().t()) * 2.0).to(BF)
    assert torch.equal(out.cpu(), ref)


def _quant(x, dev):
    from vt355 import ops
    xq, s = ops.quantize_fp8(x.to(dev, BF).contiguous())
    return xq, s, xq.double().cpu() * s.double().cpu()


_SMALL = [(e, t, 200, 384, 256) for e in ("bias", "gelu", "gated") for t in (False, True)]
_FULL = [("bias", False, 10456, 9216, 3072), ("gated", True, 10456, 9216, 3072)]       # one full block shape per tail setting


@pytest.mark.parametrize("epi,tail,M,N,K", _SMALL + _FULL)
def test_gemm_mxfp8_random_vs_fp64(dev, epi, tail, M, N, K):
    """random operands vs fp64 of the de-quantised operands, every epilogue, with and without the bf16 tail (Kt = 64).  Measured rel-L2
    (MI355X): 1.3e-3 .. 2.2e-3 -- the bf16 rounding of the outputs; the cap is 5e-3"""
    from vt355 import ops
    from vt355.ops import EPI_BIAS, EPI_BIAS_GELU, EPI_GATED_RES
    gen = torch.Generator().manual_seed(2)
    aq, sa, ad = _quant(torch.randn(M, K, generator=gen), dev)
    wq, sw, wd = _quant(torch.randn(N, K, generator=gen) * K ** -0.5, dev)
    bias = (torch.randn(N, generator=gen) * 0.1).to(BF)
    ref = (ad.to(dev) @ wd.to(dev).t()).cpu() + bias.double()
    kw = {}
    if tail:
        At = (torch.randn(M, 64, generator=gen) * 0.5).to(BF); Wt = (torch.randn(N, 64, generator=gen) * 0.1).to(BF)
        ref = ref + At.double() @ Wt.double().t()
        kw["tail"] = (At.to(dev), Wt.to(dev))
    out = poisoned((M, N), BF, dev)
    if epi == "bias":
        ops.gemm_mxfp8(aq, wq, out, sa, sw, bias.to(dev), **kw)
        assert rel_l2(out, ref) < 5e-3
    elif epi == "gelu":
        u = poisoned((M, N), BF, dev)
        ops.gemm_mxfp8(aq, wq, out, sa, sw, bias.to(dev), epilogue=EPI_BIAS_GELU, pre_act_out=u, **kw)
        assert rel_l2(u, ref) < 5e-3
        assert rel_l2(out, _gelu_tanh(ref)) < 5e-3
    else:
        S = M // 2
        R = torch.randn(M, N, generator=gen).to(BF)
        gate = torch.randn(2, 3 * N, generator=gen)                  # two samples' gates, bstride 3 N (as a modulation vector slice)
        branch = poisoned((M, N), BF, dev)
        gd = gate.to(dev)[:, :N]
        ops.gemm_mxfp8(aq, wq, out, sa, sw, bias.to(dev), epilogue=EPI_GATED_RES, residual=R.to(dev), gate_txt=gd, gate_vid=gd,
                       gate_bstride=3 * N, S=S, St=0, pre_act_out=branch, **kw)
        b_of = torch.arange(M) // S
        g = gate[:, :N].double()[b_of.clamp_max(1)]
        assert rel_l2(branch, ref) < 5e-3
        assert rel_l2(out, R.double() + g * ref) < 5e-3


@pytest.mark.parametrize("epi", ["bias", "gelu"])
def test_gemm_mxfp8_fp8_output_copy_exact(dev, epi):
    """out_fp8: Cq must be the CPU cast of the bf16 output (as written) over the scale, byte for byte, and the amax slot max |out|"""
    from vt355 import ops
    from vt355.ops import EPI_BIAS, EPI_BIAS_GELU
    gen = torch.Generator().manual_seed(3)
    M, N, K = 333, 512, 256
    aq, sa, _ = _quant(torch.randn(M, K, generator=gen), dev)
    wq, sw, _ = _quant(torch.randn(N, K, generator=gen) * K ** -0.5, dev)
    out = poisoned((M, N), BF, dev)
    cq = poisoned((M, N), F8, dev)
    sq = torch.tensor([0.0031], device=dev)
    amax = torch.zeros(1, device=dev)
    kw = dict(epilogue=EPI_BIAS_GELU, pre_act_out=poisoned((M, N), BF, dev)) if epi == "gelu" else {}
    ops.gemm_mxfp8(aq, wq, out, sa, sw, None, out_fp8=(cq, sq, amax), **kw)
    all_written(cq, "fp8 output copy", expect=_e4m3_cpu(out, sq).to(dev))
    assert torch.equal(_bytes(cq), _bytes(_e4m3_cpu(out, sq)))
    assert amax.item() == out.float().abs().max().item()
    assert (out.float().abs() > 448 * 0.0031).any()                 # some values saturate


def test_cast_fp8_scaled_exact(dev):
    """vt_cast_fp8_scaled: bytes vs the CPU cast (values above 448 * scale saturate), the amax, and the bf16 row copy through (L, Lj, off)"""
    from vt355 import ops
    gen = torch.Generator().manual_seed(4)
    B, Lj, L, off, K = 3, 50, 17, 29, 384
    x = (torch.randn(B * Lj, K, generator=gen) * 3).to(BF).to(dev)
    scale = torch.tensor([0.0057], device=dev)
    y = poisoned((B * L, K), F8, dev)
    cp = torch.full((B * L, K + 64), 5.0, dtype=BF, device=dev)
    amax = torch.zeros(1, device=dev)
    ops.cast_fp8_scaled(x, y, scale, amax, copy=cp[:, :K], rows=(L, Lj, off))
    rows = x.view(B, Lj, K)[:, off:off + L].reshape(B * L, K)
    assert torch.equal(cp[:, :K], rows) and bool((cp[:, K:] == 5.0).all())
    all_written(y, "fp8 cast", expect=_e4m3_cpu(rows, scale).to(dev))
    assert torch.equal(_bytes(y), _bytes(_e4m3_cpu(rows, scale)))
    assert amax.item() == rows.float().abs().max().item()
    assert (rows.float().abs() > 448 * 0.0057).any()
    # identity row map into a column slice of a wider buffer; the slot keeps the maximum over calls
    x2 = torch.randn(64, 256, generator=gen).to(BF).to(dev)
    y2 = torch.zeros(64, 512, dtype=F8, device=dev)
    ops.cast_fp8_scaled(x2, y2[:, 256:], scale, amax)
    assert torch.equal(_bytes(y2[:, 256:]), _bytes(_e4m3_cpu(x2, scale))) and bool((_bytes(y2[:, :256]) == 0).all())
    assert amax.item() == max(rows.float().abs().max().item(), x2.float().abs().max().item())


def test_ln_modulate_fwd_fp8_exact(dev):
    """the bf16 output equals vt_ln_modulate_fwd's bit for bit; the fp8 copy is the CPU cast of it; the amax exact"""
    ln_modulate_fwd_fp8_case(dev)


def ln_modulate_fwd_fp8_case(dev, rows=None):
    """rows: (M, D, generator) -> the bf16-representable input rows, in place of the randn ones (tests/test_conditioning_gpu.py)"""
    from vt355 import ops
    gen = torch.Generator().manual_seed(5)
    B, L, D = 2, 70, 3072
    M = B * L
    x = torch.randn(M, D, generator=gen).to(BF).to(dev)
    if rows is not None:
        x = rows(M, D, gen).to(BF).to(dev)
    modv = torch.randn(B, 6 * D, generator=gen).to(dev) * 0.3
    sh, sc = modv[:, :D], modv[:, D:2 * D]
    mod = (sh, sc, sh, sc, 6 * D)
    y0 = poisoned((M, D), BF, dev); y1 = poisoned((M, D), BF, dev)
    mean0, rstd0 = poisoned((M,), torch.float32, dev), poisoned((M,), torch.float32, dev)
    mean1, rstd1 = poisoned((M,), torch.float32, dev), poisoned((M,), torch.float32, dev)
    ops.ln_modulate_fwd(x, y0, None, None, mod, mean0, rstd0, D, L, 0, 1e-6)
    q = poisoned((M, D), F8, dev)
    qs = torch.tensor([0.0123], device=dev)
    amax = torch.zeros(1, device=dev)
    ops.ln_modulate_fwd_fp8(x, y1, None, None, mod, mean1, rstd1, D, L, 0, 1e-6, q, qs, amax)
    assert torch.equal(y0, y1) and torch.equal(mean0, mean1) and torch.equal(rstd0, rstd1)
    all_written(q, "fp8 copy of the modulated LayerNorm", expect=_e4m3_cpu(y1, qs).to(dev))
    assert torch.equal(_bytes(q), _bytes(_e4m3_cpu(y1, qs)))
    assert amax.item() == y1.float().abs().max().item()


def test_fp8_scale_update_matches_restatement(dev):
    """20 sites, 20 updates of synthetic amaxes (one site always 0, one with a single spike that must leave the window after H updates):
    rolling window (newest first), max / 448 (IEEE division, on the CPU), 1 for an all-zero history, slots cleared"""
    from vt355 import ops
    gen = torch.Generator().manual_seed(6)
    n, H, T = 20, 16, 20
    seq = torch.rand(T, n, generator=gen) * torch.logspace(-3, 3, n)
    seq[:, 3] = 0.0
    seq[:, 5] = 0.01; seq[1, 5] = 50.0
    amax = torch.zeros(n, device=dev); hist = torch.zeros(n, H, device=dev); scale = torch.zeros(n, device=dev)
    h_ref = torch.zeros(n, H)
    for t in range(T):
        amax.copy_(seq[t])
        ops.fp8_scale_update(amax, hist, scale)
        h_ref = torch.cat([seq[t][:, None], h_ref[:, :-1]], 1)
        mx = h_ref.max(1).values
        s_ref = torch.where(mx > 0, mx / 448.0, torch.ones_like(mx))
        assert torch.equal(hist.cpu(), h_ref) and torch.equal(scale.cpu(), s_ref) and bool((amax == 0).all())
    assert scale[3].item() == 1.0 and scale[5].item() == torch.tensor(0.01) / 448.0


def _rope_tables(S, gen):
    ang = torch.rand(S, 64, generator=gen) * 6.28
    return torch.repeat_interleave(ang.cos(), 2, dim=1).contiguous(), torch.repeat_interleave(ang.sin(), 2, dim=1).contiguous()


def _blocks_inputs(dev, seed):
    gen = torch.Generator().manual_seed(seed)
    B, Li, Lt, D = 2, 160, 32, 256
    img, txt, vec = torch.randn(B, Li, D, generator=gen).to(BF), torch.randn(B, Lt, D, generator=gen).to(BF), torch.randn(B, D, generator=gen).to(BF)
    cos, sin = _rope_tables(Li, gen)
    dout = torch.randn(B, Li + Lt, D, generator=gen).to(BF)
    return [t.to(dev) for t in (img, txt, vec, torch.tensor([32, 19]), cos, sin, dout)]


def test_blocks_delayed_scaling_full_finetune(dev):
    """HunyuanBlocks (D 256, 2 double + 2 single blocks = 20 activation sites), full fine-tune, fp8="mfma" vs the same weights in "weights"
    mode and in bf16.  Forward 1 scales just in time and seeds every site; the output differs from "weights" mode (the fp8 products ran) and
    stays within 8e-2 rel-L2 of bf16 (measured 1.8e-2; "weights" mode 1.4e-2).  Every Linear weight / bias gradient within 5e-2 of
    "weights" mode; the per-head q / k RMSNorm weights' gradients (sums over all rows that largely cancel) are no further from "weights" mode
    than "weights" mode is from bf16 (measured 6.7e-2 vs 8.8e-2 at worst).  An optimizer step gives finite weights.  Forward 2 with inputs and conditioning x8: finite; forward 3's history holds forward 2's amaxes
    and its scales are max(history) / 448."""
    from vt355.hunyuan import HunyuanBlocks
    from vt355.optim import FusedAdamW
    img, txt, vec, tv, cos, sin, dout = _blocks_inputs(dev, 9)
    res = {}
    for mode in (False, "weights", "mfma"):
        m = HunyuanBlocks(hidden_size=256, heads_num=2, mm_double_blocks_depth=2, mm_single_blocks_depth=2, fp8=mode).to(dev).init_weights(4)
        ts = m.enable_training()
        out = m(img, txt, vec, tv, (cos, sin))
        out.backward(dout)
        res[mode] = (out.detach().float(), {n: m._view(ts.grad, n).detach().clone() for n in m.shapes})
        if mode != "mfma":
            continue
        st = m._fp8_state
        assert m.n_fp8_sites == 20 and st.seeded
        a1 = st.history[:, 0].clone()
        assert bool((a1 > 0).all()) and torch.equal(st.scale.cpu(), a1.cpu() / 448.0)
        opt = FusedAdamW(ts.params, lr=1e-4, fullft_state=ts)
        opt.step()
        assert torch.isfinite(ts.flat).all()
        with torch.no_grad():
            o2 = m(img * 8, txt * 8, vec * 8, tv, (cos, sin))
        assert torch.isfinite(o2.float()).all()
        a2 = st.amax.clone()                                  # recorded by forward 2, rolled in by forward 3
        assert bool((a2 > 0).all()) and bool((a2 > a1).any())
        with torch.no_grad():
            o3 = m(img, txt, vec, tv, (cos, sin))
        assert torch.isfinite(o3.float()).all()
        h = st.history.cpu()
        assert torch.equal(h[:, 0], a2.cpu())
        assert torch.equal(st.scale.cpu(), h.max(1).values / 448.0)
    ob, ow, oq = res[False][0], res["weights"][0], res["mfma"][0]
    e = rel_l2(oq, ob)
    errs = sorted(((rel_l2(res["mfma"][1][n], res["weights"][1][n]), rel_l2(res["weights"][1][n], res[False][1][n]), n) for n in res["weights"][1]),
                  reverse=True)
    lin = [x for x in errs if not x[2].endswith("norm.weight")]
    norms = [x for x in errs if x[2].endswith("norm.weight")]
    print(f"[hunyuan mxfp8] output vs bf16 rel-L2 {e:.3e} (weights mode {rel_l2(ow, ob):.3e}); worst Linear gradient vs weights mode "
          f"{lin[0][2]} {lin[0][0]:.2e}; q / k norm gradients (vs weights mode, weights mode vs bf16): "
          f"{[(n, f'{a:.2e}', f'{b:.2e}') for a, b, n in norms[:4]]}")
    assert not torch.equal(oq, ow)
    assert e < 8e-2 and lin[0][0] < 5e-2 and len(norms) == 12
    assert all(a < b for a, b, _ in norms)


def test_blocks_lora_tail(dev):
    """rank-4 adapters (zero_b=False, B x 10: the adapters move the output by 12 %) on the same blocks, frozen weights, fp8="mfma" vs
    "weights" vs bf16.  The adapters' contribution out(B) - out(B = 0) in "mfma" matches "weights" mode within 0.25 rel-L2 (measured 0.14;
    "weights" vs bf16: 0.08) -- without the bf16 tail the adapted sites would contribute nothing (rel-L2 ~1).  Every adapter gradient is
    within 8e-2 of "weights" mode and no further from it than "weights" mode is from bf16 (measured worst 5.6e-2 vs 7.4e-2): the adapter
    gradients are sums over all rows, as far apart under bf16 rounding as under fp8 products."""
    from vt355.hunyuan import HunyuanBlocks
    img, txt, vec, tv, cos, sin, dout = _blocks_inputs(dev, 11)
    res = {}
    for mode in (False, "weights", "mfma"):
        m = HunyuanBlocks(hidden_size=256, heads_num=2, mm_double_blocks_depth=2, mm_single_blocks_depth=2, fp8=mode, lora_rank=4,
                          lora_alpha=2.0).to(dev).init_weights(4)
        m.lora.init_weights(5, zero_b=False)
        with torch.no_grad():                                 # adapters that move the output well above the fp8 rounding of the blocks
            for n, p in m.lora._plist.items():
                if ".lora_B" in n:
                    p.mul_(10.0)
        ts = m.enable_lora_training()
        with torch.no_grad():
            m(img, txt, vec, tv, (cos, sin))                  # mfma: seeds the history, the runs below all use delayed scales
            o_b = m(img, txt, vec, tv, (cos, sin)).float()
            saved = {n: p.detach().clone() for n, p in m.lora._plist.items() if ".lora_B" in n}
            for n in saved:
                m.lora._plist[n].zero_()
            m.lora._packed = None
            o_0 = m(img, txt, vec, tv, (cos, sin)).float()
            for n, v in saved.items():
                m.lora._plist[n].copy_(v)
            m.lora._packed = None
        out = m(img, txt, vec, tv, (cos, sin))
        out.backward(dout)
        res[mode] = (o_b - o_0, {n: m.lora._view(ts.grad, n).detach().clone() for n in m.lora.shapes}, o_b)
    contrib = rel_l2(res["mfma"][0], res["weights"][0])
    errs = sorted(((rel_l2(res["mfma"][1][n], res["weights"][1][n]), rel_l2(res["weights"][1][n], res[False][1][n]), n) for n in res["weights"][1]),
                  reverse=True)
    worst = errs[0][0]
    print(f"[hunyuan mxfp8 lora] adapter contribution vs weights mode rel-L2 {contrib:.3e} (weights vs bf16 {rel_l2(res['weights'][0], res[False][0]):.3e}; "
          f"|contribution| / |out| {res['weights'][0].norm().item() / res['weights'][2].norm().item():.3e}; out mfma vs weights "
          f"{rel_l2(res['mfma'][2], res['weights'][2]):.3e}); worst adapter gradients (vs weights, weights vs bf16) {[(n, f'{a:.2e}', f'{b:.2e}') for a, b, n in errs[:4]]}")
    assert res["weights"][0].norm().item() > 0.05 * res["weights"][2].norm().item()
    assert contrib < 0.25 and worst < 8e-2
    assert all(a < b for a, b, _ in errs)


def test_whole_model_training_steps(dev):
    """HYVideoDiffusionTransformer (2 + 2 blocks, LoRA r 4, fp8="mfma") through HunyuanVideoFlow.training_step for 5 optimizer steps on
    fixed batches and draws: every loss finite and within 2e-2 relative of the bf16 run's (measured worst 3e-3)"""
    from vt355.hunyuan import HYVideoDiffusionTransformer, HunyuanVideoFlow
    gen = torch.Generator().manual_seed(21)
    B, Lt = 2, 24
    mask = (torch.arange(Lt)[None, :] < torch.tensor([24, 13])[:, None]).long()
    batches = [{"latents": torch.randn(B, 4, 3, 8, 12, generator=gen), "prompt_embeds": torch.randn(B, Lt, 64, generator=gen).to(BF),
                "prompt_attention_mask": mask, "pooled_prompt_embeds": torch.randn(B, 32, generator=gen).to(BF)} for _ in range(5)]
    losses = {}
    for mode in (False, "mfma"):
        m = HYVideoDiffusionTransformer(in_channels=4, hidden_size=256, heads_num=2, mm_double_blocks_depth=2, mm_single_blocks_depth=2,
                                        text_states_dim=64, text_states_dim_2=32, lora_rank=4, fp8=mode).to(dev).init_weights(11)
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
        losses[mode] = ls
    rel = [abs(a - b) / abs(b) for a, b in zip(losses["mfma"], losses[False])]
    print(f"[hunyuan mxfp8 model] losses bf16 {losses[False]} mfma {losses['mfma']} worst rel {max(rel):.3e}")
    assert all(torch.isfinite(torch.tensor(v)) for v in losses["mfma"])
    assert max(rel) < 2e-2
