"""GPU parity of the dual-context (text + per-frame image) cross-attention kernels of the DynamiCrafter path (csrc/attn_dual.hip)
through the C-ABI, against the float64 two-softmax restatement in tests/dc_oracle.py on the same bf16-rounded inputs: every element,
at the tolerances test_unet_kernels_gpu.py::test_attn_small_cross uses for the single-context kernel."""
import pytest
import torch

from dc_oracle import dual_attention_ref
from parity import bf16_leaves, close, floor_report, overall_bar, poisoned, rel_l2, untouched

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GRADS = ("dq", "dk", "dv", "dk_ip", "dv_ip")


def rb(t):
    return t.to(BF).float()


def compare(got, ref, what):
    """test_attn_small_cross's bars: output rtol 2e-2 / atol 1e-2; gradients rtol 3e-2 / atol 2e-2 * max|ref|"""
    close(got["o"], ref["o"], 2e-2, 1e-2, what + " output")
    for n in GRADS:
        close(got[n], ref[n], 3e-2, 2e-2 * ref[n].abs().max().item(), what + " " + n)


def make_inputs(B, T, HW, H, Sa, Sb, seed, shared_image=False):
    g = torch.Generator().manual_seed(seed)
    D, Sq = H * 64, T * HW
    ni = B if shared_image else B * T
    return dict(q=rb(torch.randn(B, Sq, D, generator=g)), kv=rb(torch.randn(B, Sa, 2 * D, generator=g)),
                kv_ip=rb(torch.randn(ni, Sb, 2 * D, generator=g)), do=rb(torch.randn(B, Sq, D, generator=g)),
                H=H, rpf=Sq if shared_image else HW)


def _interior(buf, shape, pad_cols):
    """the tensor of `shape` inside a guard buffer: 64 guard elements in front and behind, `pad_cols` guard columns after every row"""
    rows = 1
    for n in shape[:-1]:
        rows *= n
    ld = shape[-1] + pad_cols
    assert buf.numel() == 128 + rows * ld
    return buf[64:64 + rows * ld].view(*shape[:-1], ld)[..., :shape[-1]]


def _guarded(shape, dtype, dev, pad_cols=0):
    """a poisoned flat buffer, the output tensor inside it (written whole by the kernels) and the guard layout"""
    rows = 1
    for n in shape[:-1]:
        rows *= n
    buf = poisoned((128 + rows * (shape[-1] + pad_cols),), dtype, dev)
    return buf, _interior(buf, shape, pad_cols), pad_cols


def _border_untouched(buf, shape, pad_cols, what):
    inside = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    _interior(inside, shape, pad_cols).fill_(True)
    untouched(buf, inside, what)


def run_dual(dev, x, img_scale, check_border=False):
    """launch forward and backward on x = make_inputs(...); k | v are the two halves of one [.., 2D] buffer as the UNet's fused to_k / to_v
    GEMM leaves them"""
    from vt355 import ops
    q, kv, kvi, do, H, rpf = x["q"], x["kv"], x["kv_ip"], x["do"], x["H"], x["rpf"]
    B, Sq, D = q.shape
    Sa, Sb, ni = kv.shape[1], kvi.shape[1], kvi.shape[0]
    qd, kvd, kvid, dod = q.to(dev, BF), kv.to(dev, BF), kvi.to(dev, BF), do.to(dev, BF)
    bufs = {}
    for n, shp, dt, pad in (("o", (B, Sq, D), BF, 8), ("dq", (B, Sq, D), BF, 8), ("lse", (2, B, H, Sq), torch.float32, 0),
                            ("dk", (B, Sa, D), torch.float32, 0), ("dv", (B, Sa, D), torch.float32, 0),
                            ("dk_ip", (ni, Sb, D), torch.float32, 0), ("dv_ip", (ni, Sb, D), torch.float32, 0)):
        bufs[n] = _guarded(shp, dt, dev, pad)
    v = {n: bv[1] for n, bv in bufs.items()}
    for t in v.values():
        assert t.data_ptr() % 16 == 0
    ops.attn_dual_fwd(qd, kvd[..., :D], kvd[..., D:], kvid[..., :D], kvid[..., D:], v["o"], v["lse"], H, 0.125, rpf, img_scale)
    ops.attn_dual_bwd(qd, kvd[..., :D], kvd[..., D:], kvid[..., :D], kvid[..., D:], dod, v["lse"], v["dq"], v["dk"], v["dv"],
                      v["dk_ip"], v["dv_ip"], H, 0.125, rpf, img_scale)
    torch.cuda.synchronize()
    if check_border:
        for n, (buf, view, pad) in bufs.items():
            _border_untouched(buf, tuple(view.shape), pad, f"{n}: guard border")
            assert bool(torch.isfinite(view.float()).all()), f"{n}: non-finite values"
    return {n: t.clone() for n, t in v.items()}


def reference(x, img_scale, variant="exact"):
    D = x["q"].shape[2]
    return dual_attention_ref(x["q"], x["kv"][..., :D], x["kv"][..., D:], x["kv_ip"][..., :D], x["kv_ip"][..., D:], x["H"], x["rpf"],
                              img_scale, 0.125, x["do"], variant)


# (B, T, HW, heads): the four levels of the 320x512 recipe (2560, 640, [160,] 40 rows per frame; 40 and the small ones are not multiples
# of the 32-row query tile), Sa = 77 text + Sb = 16 image keys
SHAPES = [(2, 16, 2560, 5, 77, 16), (1, 16, 640, 10, 77, 16), (2, 16, 40, 20, 77, 16), (1, 4, 36, 2, 77, 16), (2, 3, 33, 1, 77, 16),
          (1, 4, 36, 2, 80, 32),
          # one and two text key tiles (the kernels are instantiated per tile count), 144 rows per frame = 576x1024's deepest level
          (1, 2, 144, 1, 20, 5), (2, 2, 50, 2, 40, 32)]


@pytest.mark.parametrize("img_scale", [1.0, 0.5])
@pytest.mark.parametrize("B,T,HW,H,Sa,Sb", SHAPES)
def test_attn_dual_matches_fp64_two_softmax_reference(dev, B, T, HW, H, Sa, Sb, img_scale):
    x = make_inputs(B, T, HW, H, Sa, Sb, seed=HW + Sa + H)
    got = run_dual(dev, x, img_scale, check_border=True)
    compare(got, reference(x, img_scale), f"dual attention {(B, T, HW, H, Sa, Sb)} scale {img_scale}")


def test_attn_dual_one_image_set_for_all_frames(dev):
    """a context that is not 77 + t*16 long: the tokens after the 77th are ONE image set per sample (rows_per_frame = T*HW, B items)"""
    x = make_inputs(2, 4, 300, 2, 77, 27, seed=5, shared_image=True)
    assert x["kv_ip"].shape[0] == 2 and x["rpf"] == 1200
    compare(run_dual(dev, x, 1.0, check_border=True), reference(x, 1.0), "shared image keys")


def _text_only(dev, x):
    from vt355 import ops
    q, kv, do, H = x["q"], x["kv"], x["do"], x["H"]
    B, Sq, D = q.shape
    Sa = kv.shape[1]
    qd, kvd = q.to(dev, BF), kv.to(dev, BF)
    o = poisoned((B, Sq, D), BF, dev); lse = poisoned((B, H, Sq), torch.float32, dev)
    ops.attn_small_fwd(qd, kvd[..., :D], kvd[..., D:], o, lse, H, 0.125)
    dq = poisoned((B, Sq, D), BF, dev)
    dk = poisoned((B, Sa, D), torch.float32, dev); dv = poisoned((B, Sa, D), torch.float32, dev)
    ops.attn_small_bwd(qd, kvd[..., :D], kvd[..., D:], o, do.to(dev, BF), lse, dq, dk, dv, H, 0.125)
    return {"o": o, "dq": dq, "dk": dk, "dv": dv}


def test_attn_dual_image_scale_zero_is_the_text_attention(dev):
    x = make_inputs(2, 16, 40, 20, 77, 16, seed=11)
    got = run_dual(dev, x, 0.0)
    assert bool((got["dk_ip"] == 0).all()) and bool((got["dv_ip"] == 0).all())
    txt = _text_only(dev, x)
    close(got["o"], txt["o"].float().cpu(), 2e-2, 1e-2, "img_scale 0 output vs attn_small")
    for n in ("dq", "dk", "dv"):
        r = txt[n].float().cpu()
        close(got[n], r, 3e-2, 2e-2 * r.abs().max().item(), f"img_scale 0 {n} vs attn_small")


def test_attn_dual_zero_image_values_leave_the_text_output(dev):
    x = make_inputs(2, 16, 40, 20, 77, 16, seed=12)
    D = x["q"].shape[2]
    x["kv_ip"][..., D:] = 0
    x["kv_ip"][..., :D] *= 3.0                                   # whatever k_ip holds
    x["kv_ip"] = rb(x["kv_ip"])
    close(run_dual(dev, x, 1.0)["o"], _text_only(dev, x)["o"].float().cpu(), 2e-2, 1e-2, "v_ip = 0 output vs attn_small")


def test_attn_dual_frame_permutation_moves_only_the_matching_rows(dev):
    """give frame f the image keys of frame perm[f]: o and dq of a frame depend on its own image item only, so the rows of a frame equal
    those of a run in which that item sits at the frame's own place; dk_ip / dv_ip follow their items"""
    B, T, HW, H = 2, 4, 40, 3
    x = make_inputs(B, T, HW, H, 77, 16, seed=13)
    D = H * 64
    q4, do4 = x["q"].view(B, T, HW, D), x["do"].view(B, T, HW, D)
    base = run_dual(dev, x, 1.0)
    perm = torch.tensor([2, 0, 3, 1])
    # permute queries AND image items together: frame f of the new problem is frame perm[f] of the old one
    y = dict(x)
    y["q"] = q4[:, perm].reshape(B, T * HW, D).contiguous()
    y["do"] = do4[:, perm].reshape(B, T * HW, D).contiguous()
    y["kv_ip"] = x["kv_ip"].view(B, T, 16, 2 * D)[:, perm].reshape(B * T, 16, 2 * D).contiguous()
    moved = run_dual(dev, y, 1.0)
    for n in ("o", "dq"):
        assert torch.equal(moved[n].view(B, T, HW, D), base[n].view(B, T, HW, D)[:, perm.to(dev)]), n
    for n in ("dk_ip", "dv_ip"):
        assert torch.equal(moved[n].view(B, T, 16, D), base[n].view(B, T, 16, D)[:, perm.to(dev)]), n
    # ... and swapping the image items ALONE changes exactly the frames whose item changed
    z = dict(x)
    swap = torch.tensor([1, 0, 2, 3])
    z["kv_ip"] = x["kv_ip"].view(B, T, 16, 2 * D)[:, swap].reshape(B * T, 16, 2 * D).contiguous()
    sw = run_dual(dev, z, 1.0)
    o0, o1 = base["o"].view(B, T, HW, D), sw["o"].view(B, T, HW, D)
    assert torch.equal(o0[:, 2:], o1[:, 2:]) and not torch.equal(o0[:, 0], o1[:, 0]) and not torch.equal(o0[:, 1], o1[:, 1])


@pytest.mark.parametrize("B,T,HW,H", [(2, 16, 40, 20), (1, 3, 2560, 2)])
def test_attn_dual_second_launch_is_bit_identical(dev, B, T, HW, H):
    """no atomics: the chunk partials of dk / dv (and of dk_ip / dv_ip when a frame is more than one chunk) are added in a fixed order"""
    x = make_inputs(B, T, HW, H, 77, 16, seed=14)
    a, b = run_dual(dev, x, 1.0), run_dual(dev, x, 1.0)
    for n in a:
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("variant", ["joint_softmax", "frame0_image", "delta_from_o"])
def test_comparison_rejects_the_likely_wrong_kernels(dev, variant):
    """the comparison of the parity test must tell the kernel from: one joint softmax over 93 keys, every frame meeting frame 0's image
    keys, and delta = rowsum(dO * O) used for both segments"""
    x = make_inputs(2, 16, 40, 20, 77, 16, seed=40 + 77 + 20)
    got = run_dual(dev, x, 1.0)
    compare(got, reference(x, 1.0), "exact")
    with pytest.raises(AssertionError):
        compare(got, reference(x, 1.0, variant), variant)


def test_attn_dual_refuses_what_it_cannot_do(dev):
    from vt355 import ops
    x = make_inputs(1, 2, 40, 1, 77, 16, seed=1)
    D = 64
    qd, kvd, kvid = x["q"].to(dev, BF), x["kv"].to(dev, BF), x["kv_ip"].to(dev, BF)
    o = poisoned((1, 80, D), BF, dev); lse = poisoned((2, 1, 1, 80), torch.float32, dev)
    with pytest.raises(ValueError):                              # rows_per_frame does not divide the rows
        ops.attn_dual_fwd(qd, kvd[..., :D], kvd[..., D:], kvid[..., :D], kvid[..., D:], o, lse, 1, 0.125, 33)
    big = torch.zeros(1, 97, 2 * D, dtype=BF, device=dev)        # more than 96 text keys
    with pytest.raises(Exception):
        ops.attn_dual_fwd(qd, big[..., :D], big[..., D:], kvid[..., :D], kvid[..., D:], o, lse, 1, 0.125, 40)
    bigi = torch.zeros(2, 33, 2 * D, dtype=BF, device=dev)       # more than 32 image keys
    with pytest.raises(Exception):
        ops.attn_dual_fwd(qd, kvd[..., :D], kvd[..., D:], bigi[..., :D], bigi[..., D:], o, lse, 1, 0.125, 40)


# ------------------------------------------------------------------------------------------------ the DynamiCrafter UNet
def _dc_model(dev, cfg=None, seed=21):
    import dc_oracle as DC
    from vt355.unet import UNetModel
    cfg = cfg or DC.dc_tiny_config()
    m = UNetModel(in_channels=cfg.in_channels, out_channels=cfg.out_channels, model_channels=cfg.model_channels,
                  attention_resolutions=list(cfg.attention_resolutions), num_res_blocks=cfg.num_res_blocks,
                  channel_mult=list(cfg.channel_mult), dropout=0.1, num_head_channels=64, transformer_depth=1, context_dim=cfg.context_dim,
                  use_linear=True, use_checkpoint=True, temporal_conv=True, temporal_attention=True, temporal_selfatt_only=True,
                  use_relative_position=False, use_causal_attention=False, temporal_length=cfg.temporal_length,
                  addition_attention=True, img_cross_attention=True, default_fs=10, fs_condition=True)
    P = DC.dc_init_params(cfg, seed=seed)
    assert list(P) == list(m.state_dict()), "parameter names / order differ from the reference's state_dict"
    m.load_state_dict(P)
    m.to(dev)
    m.eval()            # the reference's fixtures were taken in eval mode
    Pr = {k: v.detach().float().cpu().double() for k, v in m.state_dict().items()}       # the bf16-rounded weights the device uses
    return DC, cfg, m, Pr


def _dc_golden():
    import golden_io
    g = golden_io.load("dc_unet_tiny")
    return g, {k: torch.from_numpy(g[k]) for k in ("x", "context", "t", "fs", "noise", "out", "out_default_fs", "context_shared", "out_shared")}


def test_tiny_dc_unet_forward_matches_golden_and_restatement(dev):
    """forward on the golden inputs of the REFERENCE openaimodel3d_dc.UNetModel run: vs the reference output (weights differ by bf16
    rounding) and vs the restatement on the rounded weights -- per-frame image tokens, one image set for all frames, fs=None"""
    DC, cfg, m, Pr = _dc_model(dev)
    g, T = _dc_golden()
    x, ctx, t, fs = T["x"], T["context"], T["t"], T["fs"]
    with torch.no_grad():
        out = m(x.to(dev, BF), t.to(dev), context=ctx.to(dev, BF), fs=fs.to(dev))
        ref = DC.dc_unet_forward(Pr, cfg, x.to(BF).double(), t, ctx.to(BF).double(), fs=fs)
        e_or, e_gold = rel_l2(out, ref), rel_l2(out, T["out"])
        print(f"[dc unet tiny fwd] rel-L2 vs restatement {e_or:.3e}, vs reference golden (fp32 weights) {e_gold:.3e}")
        assert e_or < 3e-2 and e_gold < 5e-2
        sh = m(x.to(dev, BF), t.to(dev), context=T["context_shared"].to(dev, BF), fs=fs.to(dev))
        e_sh = rel_l2(sh, T["out_shared"])
        print(f"[dc unet tiny fwd] one image set for all frames: rel-L2 vs reference golden {e_sh:.3e}")
        assert e_sh < 5e-2


def test_tiny_dc_unet_fs_none_is_default_fs(dev):
    """fs=None must be fs=default_fs.  What fs determines is compared bit for bit: the int64 vector the network embeds AND the embedding
    sum [B, 4*model_channels] the forward actually computed from it (UNetModel.last_emb: sinusoid -> GEMMs -> sum, the only path by which fs
    reaches the rest of the network), which a forward that ignored resolve_fs() for None would fail.  The OUTPUTS of
    two forwards cannot be compared bit for bit on this engine, whatever fs is: GroupNorm's statistics pass (csrc/groupnorm.hip, shared
    with VideoCrafter2) adds its per-block partial sums with fp32 atomics, so two identical calls already differ (measured on an MI355X,
    tiny network: rel-L2 between two identical calls 1.6e-2 -- the VideoCrafter2 network alike --, fs=None vs fs=10 1.6e-2; printed
    below, not asserted).  The output of fs=None is therefore held to the forward test's own bars against the restatement and the
    reference run at fs = default_fs = 10 (3e-2 / 5e-2), and must be far from the restatement at another fs: in float64 the restatement
    moves by 1.4e-1 between fs = 10 and fs = 500, 4.7 times the bar."""
    DC, cfg, m, Pr = _dc_model(dev)
    g, T = _dc_golden()
    B = T["x"].shape[0]
    ten = torch.full((B,), 10, dtype=torch.int64, device=dev)
    assert torch.equal(m.resolve_fs(None, B, dev), ten) and m.resolve_fs(None, B, dev).dtype == torch.int64
    assert torch.equal(m.resolve_fs(T["fs"].to(dev), B, dev), T["fs"].to(dev))
    args = (T["x"].to(dev, BF), T["t"].to(dev))
    ctx = T["context"].to(dev, BF)
    with torch.no_grad():
        a = m(*args, context=ctx)
        emb_none = m.last_emb.clone()
        b = m(*args, context=ctx, fs=ten)
        emb_ten = m.last_emb.clone()
        b2 = m(*args, context=ctx, fs=ten)
        m(*args, context=ctx, fs=ten + 1)
        emb_other = m.last_emb.clone()
    # everything fs decides in the network is the embedding sum time_embed(t) + fps_embedding(fs) (no atomics upstream): bit for bit
    assert emb_none.shape == (B, 4 * cfg.model_channels) and torch.equal(emb_none, emb_ten)
    assert not torch.equal(emb_other, emb_ten)
    with torch.no_grad():
        xr, cr = T["x"].to(BF).double(), T["context"].to(BF).double()
        ref10 = DC.dc_unet_forward(Pr, cfg, xr, T["t"], cr, fs=None, default_fs=10)
        ref500 = DC.dc_unet_forward(Pr, cfg, xr, T["t"], cr, fs=torch.full((B,), 500))
    e10, e500 = rel_l2(a, ref10), rel_l2(a, ref500)
    print(f"[dc unet fs] fs=None vs restatement at fs=10 {e10:.3e}, at fs=500 {e500:.3e}; device: two identical calls rel-L2 {rel_l2(b2, b):.3e}, "
          f"fs=None vs fs=default_fs {rel_l2(a, b):.3e}")
    assert e10 < 3e-2 and rel_l2(b, ref10) < 3e-2
    assert rel_l2(a, T["out_default_fs"]) < 5e-2
    assert e500 > 2.0 * 3e-2


def test_tiny_dc_unet_train_step_matches_restatement(dev):
    """eps-MSE loss, every parameter gradient (to_k_ip / to_v_ip and fps_embedding among them), the gradient of the image context rows as
    one more "parameter", and one AdamW step of the tiny DynamiCrafter UNet vs the fp64 restatement"""
    from vt355 import ops
    from vt355.optim import FusedAdamW
    DC, cfg, m, Pr = _dc_model(dev)
    ts = m.enable_training()
    g, T = _dc_golden()
    x, ctx, t, fs, noise = T["x"], T["context"], T["t"], T["fs"], T["noise"]
    ctx_d = ctx.to(dev, BF).requires_grad_(True)
    out = m(x.to(dev, BF), t.to(dev), context=ctx_d, fs=fs.to(dev))
    loss = poisoned((1,), torch.float32, dev); dp = poisoned(out.shape, BF, dev)
    ops.mse_loss(out.detach().contiguous(), noise.to(dev), loss, dp)
    out.backward(dp)
    for v in Pr.values():
        v.requires_grad_(True)
    ctx_r = ctx.to(BF).double().requires_grad_(True)
    ref = DC.dc_unet_forward(Pr, cfg, x.to(BF).double(), t, ctx_r, fs=fs)
    lref = ((ref - noise.double()) ** 2).mean(dim=(1, 2, 3, 4)).mean()
    lref.backward()
    assert abs(loss.item() - lref.item()) < 2e-2 * lref.item(), (loss.item(), lref.item())
    assert abs(loss.item() - float(g["loss"])) < 5e-2 * float(g["loss"])
    pairs = [(n, m._view(ts.grad, n).detach().double().cpu(), Pr[n].grad) for n in m.shapes]
    assert ctx_d.grad is not None and float(ctx_d.grad[:, :77].abs().max()) == 0.0          # text rows: frozen encoder, no gradient
    pairs.append(("d context[:, 77:]", ctx_d.grad[:, 77:].detach().double().cpu(), ctx_r.grad[:, 77:]))
    Pb = bf16_leaves(Pr)
    ctx_b = ctx.to(BF).requires_grad_(True)
    outb = DC.dc_unet_forward(Pb, cfg, x.to(BF), t, ctx_b, fs=fs)
    assert outb.dtype == BF
    ((outb.float() - noise.float()) ** 2).mean(dim=(1, 2, 3, 4)).mean().backward()
    noisy = {n: Pb[n].grad for n in m.shapes}
    noisy["d context[:, 77:]"] = ctx_b.grad[:, 77:]
    overall, ofloor, worst, bad, ratio, at = floor_report(pairs, noisy, 0.98, 0.2)
    rel_ctx = rel_l2(pairs[-1][1], pairs[-1][2])
    print(f"[dc unet tiny train] loss dev {loss.item():.6f} restatement {lref.item():.6f} golden {float(g['loss']):.6f}; grads: overall rel-L2 "
          f"{overall:.3e} (bf16 floor {ofloor:.3e}), worst per-parameter {worst:.3e}, image context {rel_ctx:.3e}, worst device / floor {ratio:.2f} at {at}")
    assert not bad, bad[:10]
    assert overall < overall_bar(5e-2, ofloor)
    assert rel_l2(pairs[-1][1], torch.from_numpy(g["grad_context"])[:, 77:]) < 0.2          # ... and vs the reference's own gradient
    opt = FusedAdamW(ts.params, lr=1e-3, fullft_state=ts)
    before = ts.flat.clone()
    opt.step()
    assert torch.isfinite(ts.flat).all() and (ts.flat - before).abs().max().item() > 0
    assert torch.equal(ts.flat_bf16.float(), ts.flat.to(BF).float())


def test_tiny_dc_unet_train_mode_adds_the_resblock_dropout_sites(dev):
    """model.train() with dropout 0.1: every ResBlock gets its out_layers dropout next to the three of its TemporalConvBlock (8 x 4 sites,
    distinct counter ranges); a pinned seed reproduces sites and counter offsets, and eval mode differs by far more than two seeded runs do"""
    DC, cfg, m, Pr = _dc_model(dev)
    m.enable_training()
    g, T = _dc_golden()
    args = (T["x"].to(dev, BF), T["t"].to(dev))
    kw = dict(context=T["context"].to(dev, BF), fs=T["fs"].to(dev))
    m.train(); m.dropout_seed = 777
    a = m(*args, **kw)
    sites = m.last_dropout_sites
    assert len(sites) == 32 and len({o for _, o, _, _ in sites}) == 32
    assert sum(1 for s in sites if s[0].endswith(".out_layers.2")) == 8
    b = m(*args, **kw)
    assert [s_[:2] for s_ in m.last_dropout_sites] == [s_[:2] for s_ in sites]          # same seed, same counter ranges: the same masks
    m.eval()
    with torch.no_grad():
        c = m(*args, **kw)
    e_same, e_eval = rel_l2(a, b), rel_l2(a, c)
    print(f"[dc unet dropout] same seed twice rel-L2 {e_same:.3e} (GroupNorm's atomics), train vs eval {e_eval:.3e}")
    # two runs with the same masks differ only by GroupNorm's summation order (1e-2 .. 3e-2 on this tiny bf16 network, see the fs test); a run
    # without the masks changes a tenth of the activations of 32 sites (measured 6.5e-1).  The masks' values are checked bit for bit in
    # test_resblock_dropout_site_matches_the_philox_oracle.
    assert e_eval > 5e-2 and e_same < 0.25 * e_eval


def test_dc_level0_spatial_transformer_at_the_recipes_full_size(dev):
    """one SpatialTransformer of the first level with the image branch at 16 x 40 x 64 x 320 (5 heads, 77 text + 16 image tokens per frame,
    context 1024) through the engine against the fp32 restatement: output, input gradient, every parameter gradient of the layer and the
    gradient of the image context -- the bars of test_unet_gpu.py::test_unet_level0_blocks_at_the_recipes_full_size"""
    import dc_oracle as DC
    import unet_oracle as UO
    from vt355.unet import _Run, _Var
    cfgf = UO.UNetConfig(in_channels=8, model_channels=320, channel_mult=(1,), num_res_blocks=1, attention_resolutions=(1,), context_dim=1024,
                         temporal_length=16)
    DC, cfg, m, Pr = _dc_model(dev, cfg=cfgf, seed=11)
    Pr = {k: v.float() for k, v in Pr.items()}            # fp32 at this size (fp64 score tensors of 16 x 5 x 2560^2 would not fit)
    ts = m.enable_training()
    layer = m.structure.input[1][1]
    assert layer.kind == "st"
    g = torch.Generator().manual_seed(31)
    B, T, H, W, C = 1, 16, 40, 64, 320
    cl = lambda x5: x5.permute(0, 2, 3, 4, 1).reshape(-1, x5.shape[1])
    x = torch.randn(B, C, T, H, W, generator=g).to(BF).float()
    ctx = torch.randn(B, 77, 1024, generator=g).to(BF).float()
    img = torch.randn(B * T, 16, 1024, generator=g).to(BF).float()
    run = _Run(m, save=True)
    xv = _Var(cl(x).to(dev, BF).contiguous())
    ctxv = _Var(ctx.to(dev, BF).view(B * 77, -1).contiguous()); ctxv.g = False
    imgv = _Var(img.to(dev, BF).view(B * T * 16, -1).contiguous())
    imgv.g32 = torch.zeros(B * T * 16, 1024, device=dev)
    yv = run.spatial_transformer(layer, xv, [B, T, H, W], ctxv, 77, (imgv, B * T, 16))
    for v in Pr.values():
        v.requires_grad_(True)
    xr, imgr = x.clone().requires_grad_(True), img.clone().requires_grad_(True)
    x4 = xr.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W)
    ref4 = DC.dc_spatial_transformer(x4, torch.cat([ctx.repeat_interleave(T, dim=0), imgr], dim=1), Pr, layer.pre, layer.heads)
    ref5 = ref4.reshape(B, T, C, H, W).permute(0, 2, 1, 3, 4)
    gy = torch.randn(ref5.shape, generator=g).to(BF).float()
    (ref5 * gy).sum().backward()
    e_out = rel_l2(yv.d, cl(ref5))
    yv.g = cl(gy).to(dev, BF).contiguous()
    while run.tape:
        run.tape.pop()()
    e_dx = rel_l2(xv.g, cl(xr.grad))
    e_img = rel_l2(imgv.g32, imgr.grad.reshape(B * T * 16, 1024))
    names = [n for n in m.shapes if n.startswith(layer.pre + ".")]
    assert any(n.endswith("to_k_ip.weight") for n in names) and any(n.endswith("to_v_ip.weight") for n in names)
    Pb = bf16_leaves({n: Pr[n] for n in names})                   # the bf16 run costs less than the fp32 one above
    ctxb = torch.cat([ctx.repeat_interleave(T, dim=0), img], dim=1).to(BF)
    refb = DC.dc_spatial_transformer(x.to(BF).permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W), ctxb, Pb, layer.pre, layer.heads)
    assert refb.dtype == BF
    (refb.reshape(B, T, C, H, W).permute(0, 2, 1, 3, 4).float() * gy).sum().backward()
    _, _, worst, bad, ratio, at = floor_report([(n, m._view(ts.grad, n), Pr[n].grad) for n in names], {n: Pb[n].grad for n in names}, -1.0, 6e-2)
    print(f"[dc st FULL SIZE {[B, T, H, W, C]}] out rel-L2 {e_out:.3e}, dx {e_dx:.3e}, image context gradient {e_img:.3e}, worst parameter gradient "
          f"{worst:.3e} over {len(names)} tensors, worst device / floor {ratio:.2f} at {at}")
    assert e_out < 2e-2 and e_dx < 4e-2 and not bad and e_img < 6e-2, bad[:8]


# ------------------------------------------------------------------------------------------------ Resampler
def _rs_model(dev, cfg=None, seed=31):
    import dc_oracle as DC
    from vt355.resampler import Resampler
    cfg = cfg or DC.RS_TINY
    m = Resampler(**cfg)
    P = DC.rs_init_params(cfg, seed=seed)
    assert list(P) == list(m.state_dict())
    m.load_state_dict(P)
    m.to(dev)
    Pr = {k: v.detach().float().cpu().double() for k, v in m.state_dict().items()}
    return DC, cfg, m, Pr


def test_resampler_forward_backward_match_golden_and_restatement(dev):
    """tiny Resampler (2 layers, 2 heads x 64, 4 queries x 4 frames, 9 image tokens): output vs the reference run and vs the restatement on
    the bf16-rounded weights, every parameter gradient vs the restatement -- the bars of the tiny UNet tests"""
    import golden_io
    DC, cfg, m, Pr = _rs_model(dev)
    ts = m.enable_training()
    g = golden_io.load("dc_resampler")
    x, gy = torch.from_numpy(g["x"]), torch.from_numpy(g["gy"])
    out = m(x.to(dev, BF))
    assert out.shape == (2, 16, 64)
    out.backward(gy.to(dev, BF))
    for v in Pr.values():
        v.requires_grad_(True)
    ref = DC.rs_forward(Pr, cfg, x.to(BF).double())
    (ref * gy.to(BF).double()).sum().backward()
    e_or, e_gold = rel_l2(out, ref), rel_l2(out, torch.from_numpy(g["y"]))
    Pb = bf16_leaves(Pr)
    refb = DC.rs_forward(Pb, cfg, x.to(BF))
    assert refb.dtype == BF
    (refb.float() * gy.to(BF).float()).sum().backward()
    overall, ofloor, worst, bad, ratio, at = floor_report([(n, m._view(ts.grad, n), Pr[n].grad) for n in m.shapes], {n: Pb[n].grad for n in m.shapes},
                                                          0.98, 0.2)
    print(f"[resampler tiny] out rel-L2 vs restatement {e_or:.3e}, vs reference golden {e_gold:.3e}; grads overall {overall:.3e} "
          f"(bf16 floor {ofloor:.3e}), worst {worst:.3e}, worst device / floor {ratio:.2f} at {at}")
    assert e_or < 3e-2 and e_gold < 5e-2
    assert not bad, bad[:10]
    assert overall < overall_bar(5e-2, ofloor)
    with torch.no_grad():
        assert rel_l2(m(x.to(dev, BF)), ref) < 3e-2          # the no-grad path


# ------------------------------------------------------------------------------------------------ the flow: Resampler -> UNet
def test_dc_flow_loss_and_resampler_gradients_through_the_unet(dev):
    """LatentVisualDiffusionFlow.loss_from with the Resampler's output as the UNet's per-frame image context (v target, use_scale 0.3,
    zero-terminal-SNR schedule, hybrid input with conditioning frame 2): loss and the gradients of EVERY Resampler parameter -- first layer
    (latents, proj_in) to last (proj_out, norm_out) -- vs the fp64 restatement.  They exist only if the UNet's gradient of the image
    context rows reaches the module that produced them.  Then one joint optimizer step moves both modules."""
    import dc_oracle as DC
    from vt355.lvdm import LatentVisualDiffusionFlow
    cfg = DC.dc_tiny_config()
    unet = dict(target="vt355.unet.UNetModel", params=dict(
        in_channels=8, out_channels=4, model_channels=cfg.model_channels, attention_resolutions=list(cfg.attention_resolutions),
        num_res_blocks=cfg.num_res_blocks, channel_mult=list(cfg.channel_mult), dropout=0.1, num_head_channels=64, transformer_depth=1,
        context_dim=cfg.context_dim, use_linear=True, use_checkpoint=True, temporal_conv=True, temporal_attention=True,
        temporal_selfatt_only=True, use_relative_position=False, use_causal_attention=False, temporal_length=cfg.temporal_length,
        addition_attention=True, img_cross_attention=True, default_fs=10, fs_condition=True))
    flow = LatentVisualDiffusionFlow(
        unet_config=unet, image_proj_stage_config=dict(target="vt355.resampler.Resampler", params=dict(DC.RS_FLOW)),
        diffusion_scheduler_config=dict(target="vt355.lvdm.LDDPM", params=dict(timesteps=1000, linear_start=0.00085, linear_end=0.012,
                                                                              rescale_betas_zero_snr=True)),
        parameterization="v", use_scale=True, scale_b=0.3, uncond_prob=0.05, uncond_type="empty_seq", rand_cond_frame=True,
        fps_condition_type="fps", image_proj_model_trainable=True, base_learning_rate=1e-3)
    flow.model.load_state_dict(DC.dc_init_params(cfg, seed=21))
    flow.image_proj_model.load_state_dict(DC.rs_init_params(DC.RS_FLOW, seed=33))
    flow.to(dev)
    flow.eval()
    opt = flow.configure_optimizers()
    uts, rts = flow.model.train_state, flow.image_proj_model.train_state
    Pu = {k: v.detach().float().cpu().double().requires_grad_(True) for k, v in flow.model.state_dict().items()}
    Pr = {k: v.detach().float().cpu().double().requires_grad_(True) for k, v in flow.image_proj_model.state_dict().items()}
    g = torch.Generator().manual_seed(17)
    B, T, H, W = 2, cfg.temporal_length, 8, 8
    z = torch.randn(B, 4, T, H, W, generator=g)
    ctx = rb(torch.randn(B, 77, cfg.context_dim, generator=g))
    tok = rb(torch.randn(B, 9, DC.RS_FLOW["embedding_dim"], generator=g))
    noise = torch.randn(B, 4, T, H, W, generator=g)
    t = torch.tensor([37, 912]); fs = torch.tensor([24, 3])
    loss = flow.loss_from(z.to(dev), ctx.to(dev, BF), tok.to(dev, BF), t.to(dev), noise.to(dev), fs.to(dev), cond_frame_index=2)
    loss.backward()
    lref = DC.dc_flow_loss(Pu, cfg, Pr, DC.RS_FLOW, z.double(), ctx.double(), tok.double(), t, noise.double(), fs, 2,
                           flow.scheduler.alphas_cumprod, flow.scale_arr.detach().cpu().double())
    lref.backward()
    assert abs(loss.item() - lref.item()) < 2e-2 * lref.item(), (loss.item(), lref.item())
    rs = flow.image_proj_model
    pairs = [(n, rs._view(rts.grad, n).detach().double().cpu(), Pr[n].grad) for n in rs.shapes]
    Pub, Prb = bf16_leaves(Pu), bf16_leaves(Pr)
    DC.dc_flow_loss(Pub, cfg, Prb, DC.RS_FLOW, z, ctx, tok, t, noise, fs, 2, flow.scheduler.alphas_cumprod.detach().cpu(),
                    flow.scale_arr.detach().cpu().float(), model_dtype=BF).backward()          # both networks in bf16, schedule / target / loss in fp32
    overall, ofloor, worst, bad, ratio, at = floor_report(pairs, {n: Prb[n].grad for n in rs.shapes}, 0.98, 0.2)
    first_last = {n: rel_l2(a, b) for n, a, b in pairs if n in ("latents", "proj_in.weight", "proj_out.weight", "norm_out.weight")}
    uo, uofloor, uw, ubad, uratio, uat = floor_report([(n, flow.model._view(uts.grad, n), Pu[n].grad) for n in flow.model.shapes],
                                                      {n: Pub[n].grad for n in flow.model.shapes}, 0.98, 0.2)
    print(f"[dc flow] loss dev {loss.item():.6f} restatement {lref.item():.6f}; Resampler grads overall {overall:.3e} (bf16 floor {ofloor:.3e}), "
          f"worst {worst:.3e}, worst device / floor {ratio:.2f} at {at}, first / last layer {first_last}; UNet grads overall {uo:.3e} "
          f"(bf16 floor {uofloor:.3e}), worst {uw:.3e}, worst device / floor {uratio:.2f} at {uat}")
    assert all(float(b.abs().max()) > 0 for _, _, b in pairs)
    assert not bad, bad[:10]
    assert overall < overall_bar(5e-2, ofloor) and not ubad and uo < overall_bar(5e-2, uofloor), ubad[:10]
    bu, br = uts.flat.clone(), rts.flat.clone()
    opt.step()
    assert torch.isfinite(uts.flat).all() and torch.isfinite(rts.flat).all()
    assert (uts.flat - bu).abs().max().item() > 0 and (rts.flat - br).abs().max().item() > 0
    # the stochastic wrapper: train mode, every sample's text AND image condition dropped or kept by the three-way rule
    flow.train()
    opt.zero_grad()
    batch = {"latents": z.to(dev), "context": ctx.to(dev, BF), "image_tokens": tok.to(dev, BF), "fps": fs.to(dev),
             "null_context": torch.zeros(77, cfg.context_dim, device=dev, dtype=BF), "null_image_tokens": torch.zeros(9, DC.RS_FLOW["embedding_dim"], device=dev, dtype=BF)}
    l2 = flow.training_step(batch)
    l2.backward()
    assert torch.isfinite(l2) and torch.isfinite(rts.grad).all() and float(rts.grad.abs().max()) > 0


def test_resblock_dropout_site_matches_the_philox_oracle(dev):
    """one ResBlock of the tiny DynamiCrafter UNet in train mode (dropout 0.1): the keep masks of its four dropout sites -- the new
    out_layers.2 site and the TemporalConvBlock's three -- are recomputed bit for bit by oracle/philox.py from the recorded (seed, counter
    offset) and handed to the restatement; output, input gradient and every parameter gradient of the layer must agree (so mask values,
    placement and the 1 / (1 - p) scale are right), and must differ from the same block without the out_layers mask"""
    import philox
    from vt355.unet import _Run, _Var
    DC, cfg, m, Pr = _dc_model(dev)
    ts = m.enable_training()
    m.train(); m.dropout_seed = 424242
    layer = m.structure.input[1][0]
    assert layer.kind == "res"
    g = torch.Generator().manual_seed(8)
    B, T, H, W, C = 2, 4, 8, 8, layer.cin
    cl = lambda x5: x5.permute(0, 2, 3, 4, 1).reshape(-1, x5.shape[1])
    x = rb(torch.randn(B, C, T, H, W, generator=g))
    se = rb(torch.nn.functional.silu(torch.randn(B, 4 * cfg.model_channels, generator=g)))
    run = _Run(m, save=True)
    assert run.drop is not None
    xv = _Var(cl(x).to(dev, BF).contiguous())
    demb = torch.zeros(B, se.shape[1], device=dev)
    yv = run.res_block(layer, xv, [B, T, H, W], _Var(se.to(dev, BF)), demb)
    sites = run.drop_sites
    assert [s[0] for s in sites] == [layer.pre + ".out_layers.2"] + [layer.pre + f".temopral_conv.conv{j}" for j in (2, 3, 4)]
    masks = {}
    for name, off, M, Cc in sites:
        k = torch.from_numpy(philox.dropout_keep_mask(M, Cc, 0.1, m.dropout_seed, off)).view(B, T, H, W, Cc)          # rows = (b, t, h, w)
        masks[name] = k.permute(0, 1, 4, 2, 3).reshape(B * T, Cc, H, W) if name.endswith("out_layers.2") else k.permute(0, 4, 1, 2, 3)
    for v in Pr.values():
        v.requires_grad_(True)
    xr = x.double().requires_grad_(True)
    x4 = xr.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W)
    ser = se.double().repeat_interleave(T, dim=0)
    ref4 = DC.dc_res_block_train(x4, ser, Pr, layer.pre, B, masks, 0.1)
    ref5 = ref4.reshape(B, T, -1, H, W).permute(0, 2, 1, 3, 4)
    gy = rb(torch.randn(ref5.shape, generator=g))
    (ref5 * gy.double()).sum().backward()
    e_out = rel_l2(yv.d, cl(ref5))
    yv.g = cl(gy).to(dev, BF).contiguous()
    while run.tape:
        run.tape.pop()()
    e_dx = rel_l2(xv.g, cl(xr.grad))
    names = [n for n in m.shapes if n.startswith(layer.pre + ".")]
    Pb = bf16_leaves({n: Pr[n] for n in names})
    refb = DC.dc_res_block_train(x.to(BF).permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W), se.to(BF).repeat_interleave(T, dim=0), Pb, layer.pre, B, masks, 0.1)
    assert refb.dtype == BF
    (refb.reshape(B, T, -1, H, W).permute(0, 2, 1, 3, 4).float() * gy).sum().backward()
    _, _, worst, bad, ratio, at = floor_report([(n, m._view(ts.grad, n), Pr[n].grad) for n in names], {n: Pb[n].grad for n in names}, -1.0, 6e-2)
    with torch.no_grad():
        nomask = dict(masks); nomask[layer.pre + ".out_layers.2"] = torch.ones_like(masks[layer.pre + ".out_layers.2"])
        e_wrong = rel_l2(yv.d, cl(DC.dc_res_block_train(x4, ser, Pr, layer.pre, B, nomask, 0.1).reshape(B, T, -1, H, W).permute(0, 2, 1, 3, 4)))
    print(f"[dc resblock train] out rel-L2 {e_out:.3e}, dx {e_dx:.3e}, worst parameter gradient {worst:.3e}, worst device / floor {ratio:.2f} at {at}; "
          f"with a wrong out_layers mask {e_wrong:.3e}")
    assert e_out < 2e-2 and e_dx < 4e-2 and not bad, bad[:8]          # test_unet_gpu.py's block bars
    assert e_wrong > 5 * e_out
