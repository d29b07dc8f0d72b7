"""HunyuanVideo blocks on the device (vt355.hunyuan) against the CPU oracle (oracle/hunyuan_oracle.py, pinned to the imported reference
MMDoubleStreamBlock / MMSingleStreamBlock by tests/golden/hunyuan_blocks.npz) -- BASELINE configs[4], SURVEY 8(a) a16."""
import os

import numpy as np
import pytest
import torch

from parity import bf16_leaves, floor_report, poisoned, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rope_tables(S, gen):
    ang = torch.rand(S, 64, generator=gen) * 6.28
    return torch.repeat_interleave(ang.cos(), 2, dim=1).contiguous(), torch.repeat_interleave(ang.sin(), 2, dim=1).contiguous()


@pytest.mark.parametrize("L,Lout,off,rope", [(24, 24, 0, True), (10, 37, 27, False), (27, 37, 0, True)])
def test_qk_rmsnorm_rope128_matches_torch(dev, L, Lout, off, rope):
    """vt_qk_rmsnorm_rope128 fwd / bwd vs a torch fp64 statement of RMSNorm (norm_layers.py:5-58) + apply_rotary_emb (posemb_layers.py:133-188)
    + the placement into the joint sequence; the rope covers the first S_rope = L - 3 positions when L == Lout (single block: text rows at
    the end are not rotated)"""
    qk_rmsnorm_rope128_case(dev, L, Lout, off, rope)


def qk_rmsnorm_rope128_case(dev, L, Lout, off, rope, rows=None):
    """rows: (B L 3 H, 128, generator) -> the bf16-representable 128-wide head rows, in place of the randn ones (tests/test_conditioning_gpu.py)"""
    import hunyuan_oracle as HO
    from vt355 import ops
    gen = torch.Generator().manual_seed(5)
    B, H = 2, 3
    C = H * 128
    S_rope = (L - 3 if L == Lout else L) if rope else 0
    qkv = torch.randn(B * L, 3 * C, generator=gen).to(BF)
    if rows is not None:
        qkv = rows(B * L * 3 * H, 128, gen).view(B * L, 3 * C).to(BF)
    gq = (1 + 0.1 * torch.randn(128, generator=gen)).to(BF); gk = (1 + 0.1 * torch.randn(128, generator=gen)).to(BF)
    cos, sin = _rope_tables(max(S_rope, 1), gen)
    dout = torch.randn(B * Lout, 3 * C, generator=gen).to(BF)
    out = torch.full((B * Lout, 3 * C), 7.0, dtype=BF, device=dev)
    rstd = poisoned((B * L, 2 * H), torch.float32, dev)
    rp = (cos.to(dev), sin.to(dev)) if rope else None
    ops.qk_rmsnorm_rope128_fwd(qkv.to(dev), out, gq.to(dev), gk.to(dev), rstd, H, L, Lout, off, rp)
    dqkv = poisoned((B * L, 3 * C), BF, dev)
    dgq = torch.zeros(128, device=dev); dgk = torch.zeros(128, device=dev)
    ops.qk_rmsnorm_rope128_bwd(dout.to(dev), qkv.to(dev), dqkv, gq.to(dev), gk.to(dev), rstd, dgq, dgk, H, L, Lout, off, rp)

    x = qkv.double().requires_grad_(True)
    wq, wk = gq.double().requires_grad_(True), gk.double().requires_grad_(True)
    q, k, v = [t.view(B, L, H, 128) for t in x.view(B, L, 3, C).unbind(2)]
    q, k = HO.rms_norm(q, wq), HO.rms_norm(k, wk)
    if rope:
        q = torch.cat([HO.rope(q[:, :S_rope], cos.double(), sin.double()), q[:, S_rope:]], 1)
        k = torch.cat([HO.rope(k[:, :S_rope], cos.double(), sin.double()), k[:, S_rope:]], 1)
    ref = torch.stack([q.reshape(B, L, C), k.reshape(B, L, C), v.reshape(B, L, C)], 2).reshape(B, L, 3 * C)
    o3 = out.view(B, Lout, 3 * C)
    assert rel_l2(o3[:, off:off + L], ref) < 6e-3
    untouched = torch.ones(Lout, dtype=torch.bool); untouched[off:off + L] = False
    assert (o3[:, untouched.to(dev)] == 7.0).all()
    (ref * dout.double().view(B, Lout, 3 * C)[:, off:off + L]).sum().backward()
    assert rel_l2(dqkv, x.grad) < 8e-3
    assert rel_l2(dgq, wq.grad) < 5e-3 and rel_l2(dgk, wk.grad) < 5e-3


def _golden():
    g = np.load(os.path.join(G, "hunyuan_blocks.npz"))
    return g, (lambda k: torch.from_numpy(g[k]))


def _blocks(dev, n_double, n_single, seed, fp8=False):
    import hunyuan_oracle as HO
    from vt355.hunyuan import HunyuanBlocks
    m = HunyuanBlocks(hidden_size=256, heads_num=2, mm_double_blocks_depth=n_double, mm_single_blocks_depth=n_single, fp8=fp8)
    pre = "double_blocks.0." if n_double else "single_blocks.0."
    shapes = HO.double_block_shapes(256, 2, pre=pre) if n_double else HO.single_block_shapes(256, 2, pre=pre)
    P = HO.init(shapes, seed)
    assert sorted(P) == sorted(k for k, _ in m.named_parameters())
    m.load_state_dict(P, strict=False)
    m.to(dev)
    Pr = {k: v.detach().float().cpu().double().requires_grad_(True) for k, v in m.named_parameters()}
    return HO, m, Pr, pre


def _b(t):
    """a bf16 leaf of the CPU restatement"""
    return t.detach().to(BF).requires_grad_(True)


def _param_grads(m, ts, Pr, tag, rerun):
    """every parameter gradient finite, cosine above 0.985 and rel-L2 below its bar against the fp64 oracle's.  rerun(Pb) runs the same oracle
    step once more on the bf16 leaves Pb with bf16 inputs (the upstream gradient meeting the bf16 output in fp32); the bars are 1.5 x that
    run's own per-parameter distance from fp64 (parity.floor_bars), never above the old flat 0.15"""
    Pb = bf16_leaves(Pr)
    rerun(Pb)
    overall, ofloor, worst, bad, ratio, at = floor_report([(n, m._view(ts.grad, n), Pr[n].grad) for n in m.shapes], {n: Pb[n].grad for n in m.shapes},
                                                          0.985, 0.15)
    print(f"[hunyuan {tag}] parameter grads: overall rel-L2 {overall:.3e} (bf16 floor {ofloor:.3e}), worst {worst:.3e}, worst device / floor {ratio:.2f} at {at}")
    assert not bad, bad[:8]
    assert overall < 1.5 * ofloor, (overall, ofloor)


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


def _lora_grads(m, ts, base, ad, D, tag, cos_min, rel_max, rerun):
    """the adapter gradients against the fp64 oracle's with floor-derived bars: rerun(Pe) runs the oracle step on the bf16 effective weights"""
    adb = bf16_leaves(ad)
    rerun(_lora_effective({k: v.detach().to(BF) for k, v in base.items()}, adb, m.lora.sites, m.lora.scaling, D))
    overall, ofloor, worst, bad, ratio, at = floor_report([(n, m.lora._view(ts.grad, n), ad[n].grad) for n in m.lora.shapes],
                                                          {n: adb[n].grad for n in m.lora.shapes}, cos_min, rel_max)
    print(f"[hunyuan {tag}] adapter grads overall rel-L2 {overall:.3e} (bf16 floor {ofloor:.3e}), worst {worst:.3e}, worst device / floor {ratio:.2f} at {at}")
    assert not bad, bad[:8]
    assert overall < 1.5 * ofloor, (overall, ofloor)
    return worst


def test_double_block_train_step_matches_oracle(dev):
    """one MMDoubleStreamBlock, forward + every gradient (img, txt, vec, all 24 parameters), on the golden's inputs (text lengths 12 and 7
    of 12), vs the fp64 oracle run on the same bf16-rounded weights and inputs"""
    g, T = _golden()
    HO, m, Pr, pre = _blocks(dev, 1, 0, seed=1)
    ts = m.enable_training()
    tv = T("txt_valid")
    img, txt, vec = [T(k).to(BF) for k in ("img", "txt", "vec")]
    Li, Lt = img.shape[1], txt.shape[1]
    xi, xt, xv = [t.to(dev).requires_grad_(True) for t in (img, txt, vec)]
    out = m(xi, xt, xv, tv.to(dev), (T("cos").to(dev), T("sin").to(dev)))
    gi, gt = T("d_gi").to(BF), T("d_gt").to(BF)                       # zero on the padding text rows
    out.backward(torch.cat([gi, gt], 1).to(dev))
    ri, rt, rv = [t.double().requires_grad_(True) for t in (img, txt, vec)]
    io, to = HO.double_block(ri, rt, rv, Pr, pre, 2, tv, T("cos").double(), T("sin").double())
    ((io * gi.double()).sum() + (to * gt.double()).sum()).backward()
    valid = (gt.abs().sum(-1, keepdim=True) > 0).double()
    e_img, e_txt = rel_l2(out[:, :Li], io), rel_l2(out[:, Li:].double().cpu() * valid, to * valid)
    print(f"[hunyuan double] fwd rel-L2 img {e_img:.3e} txt {e_txt:.3e}; vs reference golden img {rel_l2(out[:, :Li], T('d_img')):.3e}")
    assert e_img < 1e-2 and e_txt < 1e-2 and rel_l2(out[:, :Li], T("d_img")) < 2e-2
    for name, got, ref in (("dimg", xi.grad, ri.grad), ("dtxt", xt.grad, rt.grad), ("dvec", xv.grad, rv.grad)):
        e = rel_l2(got, ref)
        print(f"[hunyuan double] {name} rel-L2 {e:.3e}")
        assert e < 3e-2, name
    def rerun(Pb):
        bo, bt = HO.double_block(_b(img), _b(txt), _b(vec), Pb, pre, 2, tv, T("cos"), T("sin"))
        assert bo.dtype == BF and bt.dtype == BF
        ((bo.float() * gi.float()).sum() + (bt.float() * gt.float()).sum()).backward()
    _param_grads(m, ts, Pr, "double", rerun)


def test_single_block_train_step_matches_oracle(dev):
    g, T = _golden()
    HO, m, Pr, pre = _blocks(dev, 0, 1, seed=2)
    ts = m.enable_training()
    tv = T("txt_valid")
    img, txt, vec = [T(k).to(BF) for k in ("img", "txt", "vec")]
    Li, Lt = img.shape[1], txt.shape[1]
    xi, xt, xv = [t.to(dev).requires_grad_(True) for t in (img, txt, vec)]
    out = m(xi, xt, xv, tv.to(dev), (T("cos").to(dev), T("sin").to(dev)))
    gx = T("s_gx").to(BF)
    out.backward(gx.to(dev))
    rx = torch.cat([img, txt], 1).double().requires_grad_(True)
    rv = vec.double().requires_grad_(True)
    xo = HO.single_block(rx, rv, Pr, pre, 2, Lt, tv, T("cos").double(), T("sin").double())
    (xo * gx.double()).sum().backward()
    vm = (gx.abs().sum(-1, keepdim=True) > 0).double()
    e = rel_l2(out.double().cpu() * vm, xo * vm)
    e_ref = rel_l2(out.double().cpu() * vm, T("s_x").double() * vm)
    print(f"[hunyuan single] fwd rel-L2 {e:.3e}; vs reference golden {e_ref:.3e}")
    assert e < 1e-2 and e_ref < 2e-2
    dx = torch.cat([xi.grad, xt.grad], 1)
    assert rel_l2(dx, rx.grad) < 3e-2 and rel_l2(xv.grad, rv.grad) < 3e-2
    def rerun(Pb):
        bo = HO.single_block(_b(torch.cat([img, txt], 1)), _b(vec), Pb, pre, 2, Lt, tv, T("cos"), T("sin"))
        assert bo.dtype == BF
        (bo.float() * gx.float()).sum().backward()
    _param_grads(m, ts, Pr, "single", rerun)


def test_double_then_single_stack_and_fp8_projection(dev):
    """2 double + 2 single blocks: the stack runs forward / backward / optimizer step in bf16, in the reference's fp8 mode (fp8=True: EVERY
    block Linear's weight is E4M3 with a per-tensor scale, de-quantised for a bf16 product, fp8_optimization.py:55-101) and with the qkv
    projections on the fp8 matrix cores on top (fp8="matmul"); both stay within fp8 rounding of the bf16 run"""
    from vt355.hunyuan import HunyuanBlocks, flow_matching_loss
    from vt355.optim import FusedAdamW
    gen = torch.Generator().manual_seed(9)
    B, Li, Lt, D = 2, 48, 16, 256
    img, txt, vec = torch.randn(B, Li, D, generator=gen).to(BF), torch.randn(B, Lt, D, generator=gen).to(BF), torch.randn(B, D, generator=gen).to(BF)
    tv = torch.tensor([16, 5])
    cos, sin = _rope_tables(Li, gen)
    outs = {}
    for fp8 in (False, True, "matmul"):
        m = HunyuanBlocks(hidden_size=D, heads_num=2, mm_double_blocks_depth=2, mm_single_blocks_depth=2, fp8=fp8).to(dev).init_weights(4)
        ts = m.enable_training()
        out = m(img.to(dev), txt.to(dev), vec.to(dev), tv.to(dev), (cos.to(dev), sin.to(dev)))
        outs[fp8] = out[:, :Li].float()
        x0, noise = torch.randn(B, Li, D, generator=gen).to(dev), torch.randn(B, Li, D, generator=gen).to(dev)
        loss, dpred = flow_matching_loss(out[:, :Li].contiguous(), x0, noise)
        ref = ((out[:, :Li].float() - (noise - x0)) ** 2).mean()
        assert abs(loss.item() - ref.item()) < 1e-4 * ref.item()
        dfull = torch.zeros_like(out); dfull[:, :Li] = dpred
        out.backward(dfull)
        assert torch.isfinite(ts.grad).all() and ts.grad.abs().max().item() > 0
        opt = FusedAdamW(ts.params, lr=1e-3, fullft_state=ts)
        before = ts.flat.clone()
        opt.step()
        assert torch.isfinite(ts.flat).all() and (ts.flat - before).abs().max().item() > 0
    e1, e2 = rel_l2(outs[True], outs[False]), rel_l2(outs["matmul"], outs[False])
    print(f"[hunyuan fp8] image rows vs bf16: E4M3 weights on every block Linear rel-L2 {e1:.3e}; + fp8 qkv products {e2:.3e}")
    assert 0 < e1 < 6e-2 and 0 < e2 < 8e-2


def test_fp8_mode_is_the_bf16_model_on_dequantised_e4m3_weights(dev):
    """The reference's fp8 mode stores W as E4M3 with scale = max|W| / 448 and computes F.linear(x, dequant(W)) (fp8_optimization.py:43-78):
    a bf16 model LOADED with those de-quantised weights (the library's quantiser, checked here against a restatement with torch's
    float8_e4m3fn cast) must give the fp8=True model's output bit for bit -- every Linear of the double / single blocks (qkv, proj, MLPs, linear1 / linear2, modulation) is converted, nothing else
    (biases and the q / k norm weights are not nn.Linear weights)"""
    from vt355 import ops
    from vt355.hunyuan import HunyuanBlocks
    gen = torch.Generator().manual_seed(10)
    B, Li, Lt, D = 1, 40, 8, 256
    img, txt, vec = torch.randn(B, Li, D, generator=gen).to(BF), torch.randn(B, Lt, D, generator=gen).to(BF), torch.randn(B, D, generator=gen).to(BF)
    tv = torch.tensor([7])
    cos, sin = _rope_tables(Li, gen)
    mq = HunyuanBlocks(hidden_size=D, heads_num=2, mm_double_blocks_depth=1, mm_single_blocks_depth=1, fp8=True).to(dev).init_weights(6)
    mb = HunyuanBlocks(hidden_size=D, heads_num=2, mm_double_blocks_depth=1, mm_single_blocks_depth=1, fp8=False).to(dev).init_weights(6)
    sd, n_conv = {}, 0
    for k, v in mq.state_dict().items():
        if k in mq.shapes and k.endswith(".weight") and len(mq.shapes[k]) == 2:
            w = v.float().cpu()                                              # on the CPU: IEEE division (this torch build's GPU division is not correctly rounded)
            scale = w.abs().max() / 448.0
            restated = ((w / scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float() * scale).to(BF).to(dev)
            wq, sw = ops.quantize_fp8(v.to(dev, BF).contiguous())          # the library's quantiser: x / scale, round to nearest even
            v = (wq.float() * sw).to(BF)
            n_conv += 1
            assert sw.item() == scale.item() and torch.equal(v, restated)
        sd[k] = v
    assert n_conv == 2 * 5 + 3                 # double: (mod, qkv, proj, fc1, fc2) x (img, txt); single: linear1, linear2, modulation
    mb.load_state_dict(sd, strict=False)
    with torch.no_grad():
        oq = mq(img.to(dev), txt.to(dev), vec.to(dev), tv.to(dev), (cos.to(dev), sin.to(dev)))
        ob = mb(img.to(dev), txt.to(dev), vec.to(dev), tv.to(dev), (cos.to(dev), sin.to(dev)))
    assert torch.equal(oq, ob)


def test_sp_device_core_matches_dense_attention(dev):
    """vt355.sp.device_core (vt_attn_gen, head_dim 128, per-sample valid lengths) forward and backward vs dense fp64 attention -- the local
    attention that vt355.sp.ulysses_joint_attention wraps on the device (single rank here: the exchange itself is covered on CPU / gloo)"""
    from vt355 import sp
    gen = torch.Generator().manual_seed(3)
    B, S, h = 2, 200, 3
    q, k, v, g = [torch.randn(B, S, h, 128, generator=gen).to(BF) for _ in range(4)]
    kv_len = torch.tensor([200, 137])
    qd, kd, vd = [t.to(dev).requires_grad_(True) for t in (q, k, v)]
    out = sp.device_core(qd, kd, vd, kv_len.to(dev))
    out.backward(g.to(dev))
    qr, kr, vr = [t.double().requires_grad_(True) for t in (q, k, v)]
    s = torch.einsum("bqhd,bkhd->bhqk", qr, kr) * 128 ** -0.5
    dead = torch.arange(S)[None, :] >= kv_len[:, None]
    ref = torch.einsum("bhqk,bkhd->bqhd", s.masked_fill(dead[:, None, None, :], float("-inf")).softmax(-1), vr)
    ref.backward(g.double())
    assert rel_l2(out, ref) < 1e-2
    for a, b_, n in ((qd.grad, qr.grad, "dq"), (kd.grad, kr.grad, "dk"), (vd.grad, vr.grad, "dv")):
        assert rel_l2(a, b_) < 2e-2, n
    assert kd.grad[1, 137:].abs().max().item() == 0 and vd.grad[1, 137:].abs().max().item() == 0


@pytest.mark.parametrize("B,S,H,lens", [(2, 200, 2, (200, 137)), (1, 333, 3, None), (2, 64, 1, (1, 64)), (1, 1000, 2, (777,))])
def test_attn128_matches_dense_attention(dev, B, S, H, lens):
    """vt_attn128_fwd / _bwd (long-sequence head_dim-128 kernels) vs dense fp64 attention with per-sample valid lengths: output, log-sum-exp,
    dQ, dK, dV; ragged tiles (S not a multiple of 64 / 128), a one-key sample, keys past the valid length get zero gradients"""
    gen = torch.Generator().manual_seed(S + H)
    C = H * 128
    qkv = torch.randn(B, S, 3 * C, generator=gen).to(BF)
    g = torch.randn(B, S, C, generator=gen).to(BF)
    attn128_case(dev, qkv, g, H, lens)


def attn128_case(dev, qkv, g, H, lens):
    """qkv: bf16 [B, S, 3 H 128] fused q | k | v rows, g: bf16 [B, S, H 128] upstream gradient, lens: valid keys per sample or None.
    Forward, the one-pass (fp32 atomic dQ) and the two-pass (bf16 dQ) backward against dense fp64 attention (shared with
    tests/test_conditioning_gpu.py, which feeds it inputs that move the running maximum late in the key loop)"""
    from vt355 import ops
    B, S, C = g.shape
    g = g.clone()
    kv = None if lens is None else torch.tensor(lens, dtype=torch.int32)
    if kv is not None:
        for b in range(B):
            g[b, lens[b]:] = 0                     # padding rows carry no gradient (as in the blocks' tests)
    qd = qkv.to(dev)
    q, k, v = qd[:, :, :C], qd[:, :, C:2 * C], qd[:, :, 2 * C:]
    o = poisoned((B, S, C), BF, dev); lse = poisoned((B, H, S), torch.float32, dev)
    scale = 128 ** -0.5
    kvd = None if kv is None else kv.to(dev)
    ops.attn128_fwd(q, k, v, o, lse, H, scale, kv_len=kvd)
    dq32 = poisoned((B, S, C), torch.float32, dev); dqkv = poisoned((B, S, 3 * C), BF, dev)
    ops.attn128_bwd(q, k, v, o, g.to(dev), lse, dq32, dqkv[:, :, C:2 * C], dqkv[:, :, 2 * C:], H, scale, kv_len=kvd)
    x = qkv.double().requires_grad_(True)
    qr, kr, vr = [t.reshape(B, S, H, 128) for t in x.split(C, dim=-1)]
    s = torch.einsum("bqhd,bkhd->bhqk", qr, kr) * scale
    if kv is not None:
        dead = torch.arange(S)[None, :] >= kv[:, None].long()
        s = s.masked_fill(dead[:, None, None, :], float("-inf"))
    ref = torch.einsum("bhqk,bkhd->bqhd", s.softmax(-1), vr).reshape(B, S, C)
    ref.backward(g.double())
    valid = torch.ones(B, S, 1, dtype=torch.float64) if kv is None else (torch.arange(S)[None, :] < kv[:, None].long()).double()[..., None]
    assert rel_l2(o.double().cpu() * valid, ref * valid) < 1e-2
    lse_ref = torch.logsumexp(s, -1) * 1.4426950408889634                                         # [B, H, S], log2 domain
    vm = valid[..., 0][:, None, :]
    assert ((lse.double().cpu() - lse_ref) * vm).abs().max().item() < 2e-2
    gr = x.grad
    assert rel_l2(dq32, gr[:, :, :C]) < 2e-2                                                     # one pass: fp32 dQ accumulated atomically
    assert rel_l2(dqkv[:, :, C:2 * C], gr[:, :, C:2 * C]) < 2e-2 and rel_l2(dqkv[:, :, 2 * C:], gr[:, :, 2 * C:]) < 2e-2
    d2 = torch.full((B, S, 3 * C), 7.0, dtype=BF, device=dev)                                  # two passes: bf16 dQ written once, in place
    ops.attn128_bwd(q, k, v, o, g.to(dev), lse, d2[:, :, :C], d2[:, :, C:2 * C], d2[:, :, 2 * C:], H, scale, kv_len=kvd)
    assert rel_l2(d2[:, :, :C].double().cpu() * valid, gr[:, :, :C] * valid) < 2e-2
    assert torch.equal(d2[:, :, C:], dqkv[:, :, C:])                                           # the dK / dV pass is the same arithmetic
    if kv is not None:
        for b in range(B):
            assert dqkv[b, lens[b]:, C:].abs().max().item() == 0 if lens[b] < S else True


def test_attn128_rows_spanning_more_than_2_gib(dev):
    """The fused q|k|v buffer of the 720p x 129-frame sequence on ONE card (119 056 rows x 9216 columns, 2.19 GB) puts a head's K / V image past
    2^31 bytes; the kernels' buffer offsets are unsigned 32-bit, so up to 4 GiB is legal.  Same inputs in compact rows and in rows 5 MB apart
    (600 rows -> a 3 GB span, every row's offset past 2^31 from row 430 on): forward, log-sum-exp and the two-pass backward are bit-equal."""
    from vt355 import ops
    B, S, H = 1, 600, 2
    C = H * 128
    W = 2_500_000
    gen = torch.Generator().manual_seed(77)
    qkv = torch.randn(B, S, 3 * C, generator=gen).to(BF).to(dev)
    g = torch.randn(B, S, C, generator=gen).to(BF).to(dev)
    kv = torch.tensor([555], dtype=torch.int32, device=dev)
    g[0, 555:] = 0
    wide = poisoned((B, S, W), BF, dev)
    assert S * W * 2 > 2 ** 31 + 2 ** 29
    wide[:, :, :3 * C] = qkv
    scale = 128 ** -0.5
    res = []
    for src in (qkv, wide):
        q, k, v = src[:, :, :C], src[:, :, C:2 * C], src[:, :, 2 * C:3 * C]
        o = poisoned((B, S, C), BF, dev); lse = poisoned((B, H, S), torch.float32, dev)
        ops.attn128_fwd(q, k, v, o, lse, H, scale, kv_len=kv)
        d = torch.zeros(B, S, 3 * C, dtype=BF, device=dev)
        ops.attn128_bwd(q, k, v, o, g, lse, d[:, :, :C], d[:, :, C:2 * C], d[:, :, 2 * C:], H, scale, kv_len=kv)
        dq32 = poisoned((B, S, C), torch.float32, dev); d1 = torch.zeros(B, S, 2 * C, dtype=BF, device=dev)
        ops.attn128_bwd(q, k, v, o, g, lse, dq32, d1[:, :, :C], d1[:, :, C:], H, scale, kv_len=kv)
        res.append((o[:, :555].clone(), lse[:, :, :555].clone(), d[:, :555].clone(), d1.clone(), dq32[:, :555].clone()))
    torch.cuda.synchronize()
    for a, b in zip(res[0][:4], res[1][:4]):
        assert torch.equal(a, b)
    assert rel_l2(res[1][4], res[0][4]) < 1e-5                                                      # one pass: atomic order differs, values agree
    assert res[0][2].abs().max().item() > 0


def test_attn128_full_length_properties(dev):
    """vt_attn128 at HunyuanVideo's sequence (10 200 image + 256 text tokens, 24 heads would be 3.4 TFLOP: 4 heads here), where a dense
    reference does not fit: size-independent properties of attention and its gradient --
      * every output row is a convex combination of V rows: |o| <= max |v| per head and channel;
      * sum_i q_i . dq_i == sum_j k_j . dk_j per (sample, head)  (the scores are bilinear in q and k);
      * the backward is linear in dO: bwd(a g1 + g2) == a bwd(g1) + bwd(g2);
      * keys past the valid length get exactly zero dK / dV."""
    from vt355 import ops
    gen = torch.Generator(device=dev).manual_seed(8)
    B, S, H = 1, 10456, 4
    C = H * 128
    qkv = (0.5 * torch.randn(B, S, 3 * C, device=dev, generator=gen)).to(BF)
    q, k, v = qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:]
    kv = torch.tensor([S - 56], dtype=torch.int32, device=dev)
    o = poisoned((B, S, C), BF, dev); lse = poisoned((B, H, S), torch.float32, dev)
    scale = 128 ** -0.5
    ops.attn128_fwd(q, k, v, o, lse, H, scale, kv_len=kv)
    vmax = v[:, :S - 56].float().abs().amax(1, keepdim=True)
    assert (o.float().abs() <= vmax * 1.01 + 1e-3).all() and torch.isfinite(lse[:, :, :S - 56]).all()

    def bwd(g):
        d = poisoned((B, S, 3 * C), BF, dev)
        ops.attn128_bwd(q, k, v, o, g, lse, d[:, :, :C], d[:, :, C:2 * C], d[:, :, 2 * C:], H, scale, kv_len=kv)      # two-pass backward
        return d[:, :, :C].float(), d[:, :, C:2 * C].float(), d[:, :, 2 * C:].float()
    g1 = torch.randn(B, S, C, device=dev, generator=gen).to(BF); g2 = torch.randn(B, S, C, device=dev, generator=gen).to(BF)
    g1[:, S - 56:] = 0; g2[:, S - 56:] = 0
    dq1, dk1, dv1 = bwd(g1)
    lhs = (q.float() * dq1).view(B, S, H, 128).sum((1, 3)); rhs = (k.float() * dk1).view(B, S, H, 128).sum((1, 3))
    assert ((lhs - rhs).abs() <= 2e-2 * lhs.abs().clamp_min(1.0)).all(), (lhs, rhs)
    assert dk1[:, S - 56:].abs().max().item() == 0 and dv1[:, S - 56:].abs().max().item() == 0
    dq2, dk2, dv2 = bwd(g2)
    dq3, dk3, dv3 = bwd((2 * g1.float() + g2.float()).to(BF))
    for a, b_ in ((dq3, 2 * dq1 + dq2), (dk3, 2 * dk1 + dk2), (dv3, 2 * dv1 + dv2)):
        assert rel_l2(a, b_) < 2e-2


def test_lora_blocks_train_step_matches_oracle(dev):
    """LoRA mode (rank-4 adapters on img_attn_qkv / img_attn_proj / linear1's q, k, v rows; block weights frozen): one double + one single
    block, forward and every adapter gradient + input gradients vs the fp64 oracle run on the effective weights W + scaling * B A
    (differentiated w.r.t. A and B by autograd); the frozen weights receive no gradient buffer at all"""
    import hunyuan_oracle as HO
    from vt355.hunyuan import HunyuanBlocks
    from vt355.optim import FusedAdamW
    g, T = _golden()
    D, H, r = 256, 2, 4
    m = HunyuanBlocks(hidden_size=D, heads_num=H, mm_double_blocks_depth=1, mm_single_blocks_depth=1, lora_rank=r, lora_alpha=2.0)
    P = {**HO.init(HO.double_block_shapes(D, H, pre="double_blocks.0."), 1), **HO.init(HO.single_block_shapes(D, H, pre="single_blocks.0."), 2)}
    m.load_state_dict(P, strict=False)
    m.lora.init_weights(5, zero_b=False)
    m.to(dev)
    ts = m.enable_lora_training()
    assert m.train_state is None and ts.numel == m.lora.numel
    tv = T("txt_valid")
    img, txt, vec = [T(k).to(BF) for k in ("img", "txt", "vec")]
    Li, Lt = img.shape[1], txt.shape[1]
    xi, xt, xv = [t.to(dev).requires_grad_(True) for t in (img, txt, vec)]
    out = m(xi, xt, xv, tv.to(dev), (T("cos").to(dev), T("sin").to(dev)))
    gx = T("s_gx").to(BF)
    out.backward(gx.to(dev))
    # oracle on effective weights
    base = {k: v.detach().float().cpu().double() for k, v in m.named_parameters() if not k.startswith("lora.")}
    ad = {k[5:]: v.detach().float().cpu().double().requires_grad_(True) for k, v in m.named_parameters() if k.startswith("lora.")}
    s = m.lora.scaling
    Pe = dict(base)
    def eff(mod, rows_of):
        w = base[mod + ".weight"].clone()
        for j, t in enumerate(m.lora.sites[mod]):
            dot = "." + t if t else ""
            w[j * D:(j + 1) * D] = w[j * D:(j + 1) * D] + s * ad[f"{mod}.lora_B{dot}.weight"] @ ad[f"{mod}.lora_A{dot}.weight"]
        return w
    for mod in m.lora.sites:
        Pe[mod + ".weight"] = eff(mod, None)
    ri, rt, rv = [t.double().requires_grad_(True) for t in (img, txt, vec)]
    io, to = HO.double_block(ri, rt, rv, Pe, "double_blocks.0.", H, tv, T("cos").double(), T("sin").double())
    xo = HO.single_block(torch.cat([io, to], 1), rv, Pe, "single_blocks.0.", H, Lt, tv, T("cos").double(), T("sin").double())
    (xo * gx.double()).sum().backward()
    vm = (gx.abs().sum(-1, keepdim=True) > 0).double()
    e = rel_l2(out.double().cpu() * vm, xo * vm)
    print(f"[hunyuan lora] fwd rel-L2 {e:.3e}")
    assert e < 1e-2
    assert rel_l2(xi.grad, ri.grad) < 3e-2 and rel_l2(xt.grad.double().cpu() * (T('d_gt').abs().sum(-1, keepdim=True) > 0), rt.grad * (T('d_gt').abs().sum(-1, keepdim=True) > 0)) < 3e-2
    def rerun(Pb):
        bi, bt = HO.double_block(_b(img), _b(txt), _b(vec), Pb, "double_blocks.0.", H, tv, T("cos"), T("sin"))
        bo = HO.single_block(torch.cat([bi, bt], 1), _b(vec), Pb, "single_blocks.0.", H, Lt, tv, T("cos"), T("sin"))
        assert bo.dtype == BF
        (bo.float() * gx.float()).sum().backward()
    _lora_grads(m, ts, base, ad, D, "lora", 0.98, 0.2, rerun)
    opt = FusedAdamW(ts.params, lr=1e-3, fullft_state=ts)
    before = ts.flat.clone()
    opt.step()
    assert torch.isfinite(ts.flat).all() and (ts.flat - before).abs().max().item() > 0
    out2 = m(xi.detach(), xt.detach(), xv.detach(), tv.to(dev), (T("cos").to(dev), T("sin").to(dev)))     # repacked adapters are used
    assert (out2.float() - out.float()).abs().max().item() > 0
    # the refresh after a step rewrites only the extension columns of the stacked operands, in batched kernels: a freshly built model with
    # the same weights (packed from scratch) must give the same output bit for bit
    m2 = HunyuanBlocks(hidden_size=D, heads_num=H, mm_double_blocks_depth=1, mm_single_blocks_depth=1, lora_rank=r, lora_alpha=2.0)
    m2.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
    m2.to(dev)
    with torch.no_grad():
        out3 = m2(xi.detach(), xt.detach(), xv.detach(), tv.to(dev), (T("cos").to(dev), T("sin").to(dev)))
    assert torch.equal(out3, out2.detach())


def _model(dev, lora_rank=0):
    import hunyuan_oracle as HO
    from vt355.hunyuan import HYVideoDiffusionTransformer
    m = HYVideoDiffusionTransformer(in_channels=4, hidden_size=256, heads_num=2, mm_double_blocks_depth=1, mm_single_blocks_depth=1,
                                    text_states_dim=64, text_states_dim_2=32, lora_rank=lora_rank, lora_alpha=2.0)
    P = HO.init_model(HO.model_shapes(256, 2, 1, 1, 4, 4, (1, 2, 2), 64, 32), 3)
    m.load_state_dict(P, strict=False)
    if lora_rank:
        m.lora.init_weights(5, zero_b=False)
    m.to(dev)
    base = {k: v.detach().float().cpu().double() for k, v in m.named_parameters() if not k.startswith("lora.")}
    return HO, m, base


def test_whole_transformer_forward_matches_oracle_and_reference(dev):
    """HYVideoDiffusionTransformer (patch embed, token refiner, modulation vector, 1 + 1 blocks, final layer, unpatchify) on the device vs the
    fp64 oracle on the same bf16-rounded weights and vs the reference's own output (tests/golden/hunyuan_model.npz, fp32 weights)"""
    HO, m, base = _model(dev)
    g = np.load(os.path.join(G, "hunyuan_model.npz"))
    T = lambda k: torch.from_numpy(g[k])
    with torch.no_grad():
        out = m(T("x").to(dev), T("t").to(dev), text_states=T("text_states").to(dev), text_mask=T("text_mask").to(dev),
                text_states_2=T("text_states_2").to(dev), freqs_cos=T("cos").to(dev), freqs_sin=T("sin").to(dev), return_dict=False)
        txt = m._refine_text(T("text_states").to(dev), T("t").to(dev), T("text_mask").to(dev))
    rb = lambda k: T(k).to(BF).double()
    ref = HO.transformer_forward(base, rb("x"), T("t"), rb("text_states"), T("text_mask"), rb("text_states_2"), T("cos").double(), T("sin").double(),
                                 2, 1, 1, (1, 2, 2), 4)
    tref = HO.token_refiner(rb("text_states"), T("t"), T("text_mask"), base, 2)
    valid = T("text_mask").bool()
    e_txt = rel_l2(txt.double().cpu()[valid], tref[valid])
    e, e_gold = rel_l2(out, ref), rel_l2(out, T("out"))
    print(f"[hunyuan model] refined text rel-L2 {e_txt:.3e}; output vs oracle {e:.3e}, vs reference golden {e_gold:.3e}")
    assert tuple(out.shape) == tuple(g["out"].shape) and e_txt < 1e-2 and e < 1.5e-2 and e_gold < 2.5e-2


def test_whole_transformer_lora_training_step(dev):
    """the shipped recipe's shape of training: frozen denoiser + rank-4 adapters, flow-matching loss on the model output; adapter gradients vs
    the oracle's autograd through the whole model on the effective weights"""
    from vt355.hunyuan import flow_matching_loss
    from vt355.optim import FusedAdamW
    HO, m, base = _model(dev, lora_rank=4)
    ts = m.enable_lora_training()
    g = np.load(os.path.join(G, "hunyuan_model.npz"))
    T = lambda k: torch.from_numpy(g[k])
    gen = torch.Generator().manual_seed(3)
    x0 = torch.randn(g["x"].shape, generator=gen); noise = torch.randn(g["x"].shape, generator=gen)
    sigma = torch.tensor([0.3, 0.8])
    xt, target = HO.flow_matching(x0, noise, sigma)
    xt = xt.to(BF)
    out = m(xt.to(dev), (sigma * 1000).to(dev), text_states=T("text_states").to(dev), text_mask=T("text_mask").to(dev),
            text_states_2=T("text_states_2").to(dev), freqs_cos=T("cos").to(dev), freqs_sin=T("sin").to(dev), return_dict=False)
    loss, dpred = flow_matching_loss(out.contiguous().view(2, -1), x0.view(2, -1).to(dev), noise.view(2, -1).to(dev))
    out.backward(dpred.view(out.shape))
    ad = {k[5:]: v.detach().float().cpu().double().requires_grad_(True) for k, v in m.named_parameters() if k.startswith("lora.")}
    Pe = dict(base)
    D, s = 256, m.lora.scaling
    for mod, tags in m.lora.sites.items():
        w = base[mod + ".weight"].clone()
        for j, tg in enumerate(tags):
            dot = "." + tg if tg else ""
            w[j * D:(j + 1) * D] = w[j * D:(j + 1) * D] + s * ad[f"{mod}.lora_B{dot}.weight"] @ ad[f"{mod}.lora_A{dot}.weight"]
        Pe[mod + ".weight"] = w
    rb = lambda k: T(k).to(BF).double()
    ref = HO.transformer_forward(Pe, xt.double(), sigma * 1000, rb("text_states"), T("text_mask"), rb("text_states_2"), T("cos").double(),
                                 T("sin").double(), 2, 1, 1, (1, 2, 2), 4)
    lref = ((ref - target.double()) ** 2).mean()
    lref.backward()
    print(f"[hunyuan model lora] loss dev {loss.item():.5f} oracle {lref.item():.5f}")
    assert abs(loss.item() - lref.item()) < 2e-2 * lref.item()
    def rerun(Pb):
        bo = HO.transformer_forward(Pb, xt, sigma * 1000, T("text_states").to(BF), T("text_mask"), T("text_states_2").to(BF), T("cos"), T("sin"),
                                    2, 1, 1, (1, 2, 2), 4)
        assert bo.dtype == BF
        ((bo.float() - target) ** 2).mean().backward()
    _lora_grads(m, ts, base, ad, D, "model lora", 0.97, 0.25, rerun)
    opt = FusedAdamW(ts.params, lr=1e-3, fullft_state=ts)
    before = ts.flat.clone()
    opt.step()
    assert torch.isfinite(ts.flat).all() and (ts.flat - before).abs().max().item() > 0
    with pytest.raises(NotImplementedError):
        m.enable_training()


def test_hunyuan_flow_training_step(dev):
    """HunyuanVideoFlow.training_step (hunyuanvideo.py:883-971): sigma from the table, x_t, flow-matching loss, backward into the adapters,
    optimizer step; loss_from with a fixed sigma / noise equals the formula evaluated on the model's own output"""
    from vt355.hunyuan import HunyuanVideoFlow
    HO, m, base = _model(dev, lora_rank=4)
    flow = HunyuanVideoFlow(model=m, learning_rate=1e-3).to(dev)
    opt = flow.configure_optimizers()
    g = np.load(os.path.join(G, "hunyuan_model.npz"))
    T = lambda k: torch.from_numpy(g[k]).to(dev)
    batch = {"latents": T("x"), "prompt_embeds": T("text_states"), "prompt_attention_mask": T("text_mask"), "pooled_prompt_embeds": T("text_states_2")}
    torch.manual_seed(0)
    loss = flow.training_step(batch)
    loss.backward()
    ts = m.lora.train_state
    assert torch.isfinite(loss) and ts.grad.abs().max().item() > 0
    opt.step()
    sigma = torch.tensor([0.25, 0.75], device=dev)
    noise = torch.randn(g["x"].shape, device=dev)
    l2 = flow.loss_from(batch["latents"], batch["prompt_embeds"], batch["prompt_attention_mask"], batch["pooled_prompt_embeds"], sigma, noise)
    with torch.no_grad():
        s5 = sigma.view(-1, 1, 1, 1, 1)
        xt = ((1 - s5) * batch["latents"] + s5 * noise).to(BF)
        cos, sin = flow._rope[(3, 4, 6)]
        out = m(xt, (sigma * 1000).long(), text_states=batch["prompt_embeds"], text_mask=batch["prompt_attention_mask"],
                text_states_2=batch["pooled_prompt_embeds"], freqs_cos=cos, freqs_sin=sin, return_dict=False)
        want = ((out.float() - (noise - batch["latents"])) ** 2).mean()
    assert abs(l2.item() - want.item()) < 1e-4 * want.item()


def test_full_width_lora_blocks_train_step(dev):
    """The model's real width -- hidden 3072, 24 heads x 128, MLP 12288 -- one double + one single block in the shipped recipe's LoRA mode (rank 4,
    frozen block weights), 4 x 16 x 16 = 1024 image tokens + 64 text tokens (valid 64 / 40), B = 2: forward, input gradients and every adapter
    gradient vs the fp32 oracle on the effective weights.  The tiny-model tests pin the composition; this one exercises the GEMM tilings, the
    K-extended LoRA operands and the attention at the shapes the benchmark runs."""
    import hunyuan_oracle as HO
    from vt355.hunyuan import HunyuanBlocks, rope_tables
    D, H, r = 3072, 24, 4
    B, Li, Lt = 2, 1024, 64
    m = HunyuanBlocks(hidden_size=D, heads_num=H, mm_double_blocks_depth=1, mm_single_blocks_depth=1, lora_rank=r, lora_alpha=4.0)
    P = {**HO.init(HO.double_block_shapes(D, H, pre="double_blocks.0."), 1), **HO.init(HO.single_block_shapes(D, H, pre="single_blocks.0."), 2)}
    m.load_state_dict(P, strict=False)
    m.lora.init_weights(5, zero_b=False)
    m.to(dev)
    ts = m.enable_lora_training()
    g = torch.Generator().manual_seed(31)
    img, txt = (torch.randn(B, Li, D, generator=g) * 0.5).to(BF), (torch.randn(B, Lt, D, generator=g) * 0.5).to(BF)
    vec = torch.randn(B, D, generator=g).to(BF)
    tv = torch.tensor([64, 40])
    cos, sin = rope_tables((4, 16, 16))
    gx = (torch.randn(B, Li + Lt, D, generator=g) * 0.1).to(BF)
    gx[1, Li + 40:] = 0
    xi, xt, xv = [t.to(dev).requires_grad_(True) for t in (img, txt, vec)]
    out = m(xi, xt, xv, tv.to(dev), (cos.to(dev), sin.to(dev)))
    out.backward(gx.to(dev))
    torch.cuda.synchronize()
    base = {k: v.detach().float().cpu() for k, v in m.named_parameters() if not k.startswith("lora.")}
    ad = {k[5:]: v.detach().float().cpu().requires_grad_(True) for k, v in m.named_parameters() if k.startswith("lora.")}
    s = m.lora.scaling
    Pe = dict(base)
    for mod, tags in m.lora.sites.items():
        w = base[mod + ".weight"].clone()
        for j, t in enumerate(tags):
            dot = "." + t if t else ""
            w[j * D:(j + 1) * D] = w[j * D:(j + 1) * D] + s * ad[f"{mod}.lora_B{dot}.weight"] @ ad[f"{mod}.lora_A{dot}.weight"]
        Pe[mod + ".weight"] = w
    ri, rt, rv = [t.float().requires_grad_(True) for t in (img, txt, vec)]
    io, to = HO.double_block(ri, rt, rv, Pe, "double_blocks.0.", H, tv, cos, sin)
    xo = HO.single_block(torch.cat([io, to], 1), rv, Pe, "single_blocks.0.", H, Lt, tv, cos, sin)
    (xo * gx.float()).sum().backward()
    vm = torch.ones(B, Li + Lt, 1); vm[1, Li + 40:] = 0
    e_out = rel_l2(out.float().cpu() * vm, xo * vm)
    e_img, e_vec = rel_l2(xi.grad, ri.grad), rel_l2(xv.grad, rv.grad)
    e_txt = rel_l2(xt.grad.float().cpu() * vm[:, Li:], rt.grad * vm[:, Li:])
    def rerun(Pb):
        bi, bt = HO.double_block(_b(img), _b(txt), _b(vec), Pb, "double_blocks.0.", H, tv, cos, sin)
        bo = HO.single_block(torch.cat([bi, bt], 1), _b(vec), Pb, "single_blocks.0.", H, Lt, tv, cos, sin)
        assert bo.dtype == BF
        (bo.float() * gx.float()).sum().backward()
    worst = _lora_grads(m, ts, base, ad, D, "full width", 0.98, 0.2, rerun)       # the bf16 restatement costs less than the fp32 run above
    print(f"[hunyuan full width] fwd rel-L2 {e_out:.3e}; dimg {e_img:.3e} dtxt {e_txt:.3e} dvec {e_vec:.3e}; adapter grads worst rel-L2 {worst:.3e}")
    assert e_out < 1e-2 and e_img < 3e-2 and e_txt < 3e-2 and e_vec < 3e-2


# ------------------------------------------------------------------------------------------------ BASELINE configs[4] at its stated size
def test_attn128_720p_sequence_one_ranks_heads(dev):
    """HunyuanVideo-T2V 720p x 129 frames (BASELINE configs[4]; models.py:132-252): 33 x 45 x 80 = 118 800 image tokens + 256 text tokens =
    119 056 rows.  Under the 8-way Ulysses exchange a rank runs vt_attn128 over ALL rows for 24 / 8 = 3 heads -- this launch.  A dense
    reference does not fit, so parity is stated on SAMPLED rows and keys, exactly: 48 query rows (first / last / text / random) against fp64
    softmax(q K^T) V and their dQ; 32 keys' dK / dV against fp64 sums over all 119 056 queries (using the kernel's log-sum-exp, itself checked
    on the sampled rows); and two identities over the whole tensors: sum_j dV_j = sum_i dO_i (rows of P sum to one) and sum_j dK_j = 0
    (rows of dS sum to zero).  Keys past the valid length get zero gradients."""
    from vt355 import ops
    gen = torch.Generator(device=dev).manual_seed(720)
    B, H, Li, Lt = 1, 3, 33 * 45 * 80, 256
    S = Li + Lt
    assert S == 119056
    valid = S - 77                                    # 179 valid text tokens
    C = H * 128
    qkv = (0.6 * torch.randn(B, S, 3 * C, device=dev, generator=gen)).to(BF)
    q, k, v = qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:]
    kv = torch.tensor([valid], dtype=torch.int32, device=dev)
    o = poisoned((B, S, C), BF, dev); lse = poisoned((B, H, S), torch.float32, dev)
    scale = 128 ** -0.5
    ops.attn128_fwd(q, k, v, o, lse, H, scale, kv_len=kv)
    g = torch.randn(B, S, C, device=dev, generator=gen).to(BF)
    g[:, valid:] = 0
    d = poisoned((B, S, 3 * C), BF, dev)
    ops.attn128_bwd(q, k, v, o, g, lse, d[:, :, :C], d[:, :, C:2 * C], d[:, :, 2 * C:], H, scale, kv_len=kv)
    torch.cuda.synchronize()
    assert torch.isfinite(d.float()).all() and torch.isfinite(o[:, :valid].float()).all()
    assert d[:, valid:, C:].abs().max().item() == 0                      # padding keys: no gradient
    cpu = lambda t: t[0].double().cpu()
    qc, kc, vc, oc, gc = cpu(q), cpu(k), cpu(v), cpu(o), cpu(g)
    dqc, dkc, dvc = cpu(d[:, :, :C]), cpu(d[:, :, C:2 * C]), cpu(d[:, :, 2 * C:])
    lsec = lse[0].double().cpu()
    rg = torch.Generator().manual_seed(1)
    rows = torch.cat([torch.tensor([0, 1, Li - 1, Li, valid - 1]), torch.randint(0, valid, (43,), generator=rg)])
    keys = torch.cat([torch.tensor([0, Li - 1, Li, valid - 1]), torch.randint(0, valid, (28,), generator=rg)])
    worst = {}
    for h in range(H):
        sl = slice(128 * h, 128 * h + 128)
        Kh, Vh, Qh, Gh, Oh = kc[:valid, sl], vc[:valid, sl], qc[:, sl], gc[:, sl], oc[:, sl]
        s = (qc[rows, sl] @ Kh.t()) * scale                                # [48, valid]
        p = s.softmax(-1)
        o_ref = p @ Vh
        lse_ref = torch.logsumexp(s, -1) * 1.4426950408889634
        dlt = (gc[rows, sl] * o_ref).sum(-1, keepdim=True)
        dp = gc[rows, sl] @ Vh.t()
        dq_ref = (p * (dp - dlt)) @ Kh * scale
        e_o = ((oc[rows, sl] - o_ref).norm() / o_ref.norm()).item()
        e_l = (lsec[h, rows] - lse_ref).abs().max().item()
        e_q = ((dqc[rows, sl] - dq_ref).norm() / dq_ref.norm()).item()
        # sampled keys: column of P over ALL valid queries from the kernel's own log-sum-exp and output (delta = dO . O)
        scol = (Qh[:valid] @ kc[keys, sl].t()) * (scale * 1.4426950408889634)          # [valid, 32], log2 domain
        pcol = torch.exp2(scol - lsec[h, :valid, None])
        dlt_all = (Gh[:valid] * Oh[:valid]).sum(-1, keepdim=True)
        dv_ref = pcol.t() @ Gh[:valid]
        dpc = Gh[:valid] @ vc[keys, sl].t()
        dk_ref = (pcol * (dpc - dlt_all)).t() @ Qh[:valid] * scale
        e_v = ((dvc[keys, sl] - dv_ref).norm() / dv_ref.norm()).item()
        e_k = ((dkc[keys, sl] - dk_ref).norm() / dk_ref.norm()).item()
        worst[h] = (e_o, e_l, e_q, e_v, e_k)
        assert e_o < 1e-2 and e_l < 2e-2 and e_q < 2e-2 and e_v < 2e-2 and e_k < 3e-2, (h, worst[h])
        # identities over the whole head
        sum_dv, sum_g = dvc[:valid, sl].sum(0), Gh[:valid].sum(0)
        assert ((sum_dv - sum_g).norm() / sum_g.norm()).item() < 1e-2
        assert dkc[:valid, sl].sum(0).norm().item() < 2e-2 * dkc[:valid, sl].abs().sum(0).norm().item()
    print("[attn128 720p, 119056 rows x 3 heads] per head (o, lse2 abs, dq, dv, dk) errors on sampled rows / keys: "
          + "; ".join(f"h{h}: " + " ".join(f"{x:.2e}" for x in worst[h]) for h in range(H)))


def test_double_block_on_one_eighth_of_the_720p_rows(dev):
    """One MMDoubleStreamBlock at the model's width (3072, 24 heads x 128, MLP 12288; models.py:132-252) on one sequence-parallel rank's rows of
    the 720p sequence: 118 800 / 8 = 14 850 image rows (the first eighth of the 33 x 45 x 80 grid, its rotary rows) + 256 text rows, LoRA mode.
    Forward vs the fp32 oracle on the effective weights; the backward (too heavy for the CPU at this size) through its linearity in the
    output gradient and finite, non-zero adapter gradients."""
    import hunyuan_oracle as HO
    from vt355.hunyuan import HunyuanBlocks, rope_tables
    D, H, r = 3072, 24, 4
    B, Li, Lt = 1, 33 * 45 * 80 // 8, 256
    assert Li == 14850
    m = HunyuanBlocks(hidden_size=D, heads_num=H, mm_double_blocks_depth=1, mm_single_blocks_depth=0, lora_rank=r, lora_alpha=4.0)
    P = HO.init(HO.double_block_shapes(D, H, pre="double_blocks.0."), 1)
    m.load_state_dict(P, strict=False)
    m.lora.init_weights(5, zero_b=False)
    m.to(dev)
    ts = m.enable_lora_training()
    g = torch.Generator().manual_seed(33)
    img, txt = (torch.randn(B, Li, D, generator=g) * 0.5).to(BF), (torch.randn(B, Lt, D, generator=g) * 0.5).to(BF)
    vec = torch.randn(B, D, generator=g).to(BF)
    tv = torch.tensor([179])
    cos, sin = rope_tables((33, 45, 80))
    cos, sin = cos[:Li].contiguous(), sin[:Li].contiguous()

    def run(gx):
        ts.grad.zero_()
        xi, xt, xv = [t.to(dev).requires_grad_(True) for t in (img, txt, vec)]
        out = m(xi, xt, xv, tv.to(dev), (cos.to(dev), sin.to(dev)))
        out.backward(gx.to(dev))
        torch.cuda.synchronize()
        return out.detach(), xi.grad.float(), xv.grad.float(), ts.grad.clone()
    g1 = (torch.randn(B, Li + Lt, D, generator=g) * 0.1).to(BF); g2 = (torch.randn(B, Li + Lt, D, generator=g) * 0.1).to(BF)
    g1[:, Li + 179:] = 0; g2[:, Li + 179:] = 0
    out, di1, dv1, ga1 = run(g1)
    _, di2, dv2, ga2 = run(g2)
    _, di3, dv3, ga3 = run((2 * g1.float() + g2.float()).to(BF))
    assert torch.isfinite(out.float()).all() and torch.isfinite(ga1).all() and ga1.abs().max().item() > 0
    for a, b_ in ((di3, 2 * di1 + di2), (dv3, 2 * dv1 + dv2), (ga3, 2 * ga1 + ga2)):
        assert rel_l2(a, b_) < 3e-2
    base = {k: v.detach().float().cpu() for k, v in m.named_parameters() if not k.startswith("lora.")}
    ad = {k[5:]: v.detach().float().cpu() for k, v in m.named_parameters() if k.startswith("lora.")}
    Pe = dict(base)
    for mod, tags in m.lora.sites.items():
        w = base[mod + ".weight"].clone()
        for j, t in enumerate(tags):
            dot = "." + t if t else ""
            w[j * D:(j + 1) * D] += m.lora.scaling * ad[f"{mod}.lora_B{dot}.weight"] @ ad[f"{mod}.lora_A{dot}.weight"]
        Pe[mod + ".weight"] = w
    with torch.no_grad():
        io, to = HO.double_block(img.float(), txt.float(), vec.float(), Pe, "double_blocks.0.", H, tv, cos, sin)
    ref = torch.cat([io, to], 1)
    vm = torch.ones(B, Li + Lt, 1); vm[:, Li + 179:] = 0
    e = rel_l2(out.float().cpu() * vm, ref * vm)
    print(f"[hunyuan double block, 14850 + 256 rows at width 3072] forward rel-L2 vs oracle {e:.3e}")
    assert e < 1e-2
