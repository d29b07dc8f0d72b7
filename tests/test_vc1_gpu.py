"""GPU: temporal attention with relative-position tables (csrc/attn_relpos.hip) against the float64 restatement tests/relpos_ref.py, and
the VideoCrafter1 layout of the UNet (use_relative_position=True, temporal_conv=False) against the reference's own module
(tests/golden/vc1_*.npz, written by tests/golden/make_golden_vc1.py).

Kernel tolerances are the project's own for the packed temporal attention (test_unet_kernels_gpu.py::test_attn_small_packed_sequences):
o 2e-2 / 1e-2; dq | dk | dv 3e-2 / 2e-2 max|ref|; table gradients 3e-2 / 2e-2 max|ref of that table|; lse2 1e-3 / 2e-2.  The CPU suite
(test_vc1_cpu.py) checks on the SAME inputs that every wrong variant of relpos_ref lands far outside these bars."""
import functools
import os

import pytest
import torch

import relpos_ref as RR
from parity import close, poisoned, untouched

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32


@functools.lru_cache(maxsize=None)
def _reference(case):
    return RR.case_reference(*case)


def _zero_ref_scale(r, other):
    """test_unet_kernels_gpu._zero_ref_scale: a gradient whose own reference is identically zero (T = 1) is held to the scale of the
    gradient that carries the same factors (dv for dq / dk, the v table's for the k table's)"""
    return r.abs().max().item() or other.abs().max().item()


def _run(dev, case, tables=None, want_tables=True, d_rel=None):
    """forward + backward of one case on the device; every output the kernels write whole is poisoned first"""
    from vt355 import ops
    R, T, H, P = case
    D = H * 64
    qkv, do, rel_k, rel_v = RR.case_inputs(*case)
    if tables is not None:
        rel_k, rel_v = tables
    d = qkv.to(dev, BF)
    ek, ev = rel_k.to(dev, BF), rel_v.to(dev, BF)
    o = poisoned((R, D), BF, dev); lse = poisoned((H, R), F32, dev)
    ops.attn_relpos_fwd(d[:, :D], d[:, D:2 * D], d[:, 2 * D:], ek, ev, o, lse, H, T, 0.125)
    dqkv = poisoned((R, 3 * D), BF, dev)
    if d_rel is None and want_tables:
        d_rel = (torch.zeros(2 * P + 1, 64, dtype=F32, device=dev), torch.zeros(2 * P + 1, 64, dtype=F32, device=dev))
    dk_, dv_ = d_rel if want_tables else (None, None)
    ops.attn_relpos_bwd(d[:, :D], d[:, D:2 * D], d[:, 2 * D:], ek, ev, o, do.to(dev, BF), lse, dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:],
                        dk_, dv_, H, T, 0.125)
    return dict(o=o, lse2=lse, dqkv=dqkv, d_rel_k=dk_, d_rel_v=dv_, qkv=d, do=do.to(dev, BF), rel_v=ev)


def _check(got, ref, case, rows=None):
    R, T, H, P = case
    D = H * 64
    rows = slice(0, R) if rows is None else rows
    close(got["o"][rows], ref["o"][rows], 2e-2, 1e-2, f"{case} o")
    close(got["lse2"][:, rows], ref["lse2"][:, rows], 1e-3, 2e-2, f"{case} lse2")
    gref = torch.cat([ref["dq"], ref["dk"], ref["dv"]], 1)
    if T == 1:
        sc = ref["dv"].abs().max().item()
        assert ref["dq"].abs().max().item() == 0.0 and ref["dk"].abs().max().item() == 0.0 and ref["d_rel_k"].abs().max().item() == 0.0
        close(got["dqkv"][:, :2 * D], gref[:, :2 * D], 3e-2, 2e-2 * sc, f"{case} dq | dk at T = 1")
        close(got["dqkv"][:, 2 * D:], ref["dv"], 3e-2, 2e-2 * sc, f"{case} dv")
    else:
        close(got["dqkv"][rows], gref[rows], 3e-2, 2e-2 * gref[rows].abs().max().item(), f"{case} dq | dk | dv")
    for n, other in (("d_rel_k", "d_rel_v"), ("d_rel_v", "d_rel_k")):
        close(got[n], ref[n], 3e-2, 2e-2 * _zero_ref_scale(ref[n], ref[other]), f"{case} {n}")
    if T <= P:          # no clamp is live: the two end rows of each table are never addressed
        for n in ("d_rel_k", "d_rel_v"):
            assert bool((got[n][0] == 0).all()) and bool((got[n][2 * P] == 0).all()), f"{case} {n}: rows 0 and 2P must stay exactly zero"


@pytest.mark.parametrize("case", RR.CASES, ids=lambda c: "x".join(map(str, c)))
def test_attn_relpos_parity(dev, case):
    """(R, T, H, P): two full items at the recipe's T = P = 16; a tail item of 2 1/2 tiles whose last tile holds one sequence; T = 32 > P
    (clamp live, |j - i| up to 31, a 128-row item plus a 32-row tail); P < T with four sequences per tile and a tail; T = 4 (only distances
    +-3 used, eight heads share the tables); T = 2 with P = 1 and a two-row tail; T = 1, where the softmax is the constant 1"""
    R, T, H, P = case
    D = H * 64
    got = _run(dev, case)
    ref = _reference(case)
    _check(got, ref, case)
    if T == 1:
        v = got["qkv"][:, 2 * D:].float().view(R, H, 64)
        want = (v + got["rel_v"][P].float()).to(BF).view(R, D)
        assert torch.equal(got["o"], want), "T = 1: o must be v + Ev[P] to bf16 rounding"
        assert torch.equal(got["dqkv"][:, 2 * D:], got["do"]), "T = 1: dv must equal dO bit for bit"
        close(got["d_rel_v"][P], got["do"].double().view(R * H, 64).sum(0), 1e-5, 1e-4, "T = 1: dEv[P] = sum of dO")


def test_attn_relpos_first_level_size_reduces_tables_across_workgroups(dev):
    """the VideoCrafter2 first-level size (2560 sequences x 5 heads, 320 items): o and dq | dk | dv are compared on the last 2048 rows and
    must be finite everywhere; both table gradients are compared WHOLE against the float64 sum over all sequences and heads -- the case
    that exercises the reduction across waves, workgroups and workspace copies"""
    case = RR.BIG_CASE
    R = case[0]
    got = _run(dev, case)
    _check(got, _reference(case), case, rows=slice(R - 2048, R))
    for n in ("o", "dqkv", "lse2"):
        assert bool(torch.isfinite(got[n].float()).all()), n


def test_attn_relpos_table_gradients_accumulate(dev):
    """the kernels ADD into d_rel_*: a second backward into the same buffers gives twice the first (fp32 atomics: to 1e-5 relative)"""
    case = (256, 16, 2, 16)
    first = _run(dev, case)
    one = (first["d_rel_k"].clone(), first["d_rel_v"].clone())
    second = _run(dev, case, d_rel=(first["d_rel_k"], first["d_rel_v"]))
    for a, b, n in ((second["d_rel_k"], one[0], "d_rel_k"), (second["d_rel_v"], one[1], "d_rel_v")):
        close(a, 2.0 * b.double(), 1e-5, 1e-5 * b.abs().max().item(), f"accumulated {n}")


@pytest.mark.parametrize("case", [(80, 16, 1, 16), (160, 32, 2, 16)], ids=lambda c: "x".join(map(str, c)))
def test_attn_relpos_frozen_tables(dev, case):
    """d_rel_* = None (LoRA: the tables are frozen base weights): dq | dk | dv are bit-identical to the call that also wants the tables"""
    a = _run(dev, case)
    b = _run(dev, case, want_tables=False)
    assert torch.equal(a["dqkv"], b["dqkv"]) and torch.equal(a["o"], b["o"])


def test_attn_relpos_refuses_bad_shapes_and_writes_nothing(dev):
    from vt355 import ops
    from vt355._lib import VtError
    for R, T, P in ((96, 3, 16), (64, 16, 0), (40, 16, 16)):           # 32 % T != 0; P < 1; R % T != 0
        D = 64
        x = torch.zeros(R, 3 * D, dtype=BF, device=dev)
        ek = torch.zeros(2 * P + 1, 64, dtype=BF, device=dev)
        o = poisoned((R, D), BF, dev); lse = poisoned((1, R), F32, dev); dqkv = poisoned((R, 3 * D), BF, dev)
        dt = (poisoned((2 * P + 1, 64), F32, dev), poisoned((2 * P + 1, 64), F32, dev))
        with pytest.raises(VtError, match="vt_attn_relpos_fwd"):
            ops.attn_relpos_fwd(x[:, :D], x[:, D:2 * D], x[:, 2 * D:], ek, ek, o, lse, 1, T, 0.125)
        with pytest.raises(VtError, match="vt_attn_relpos_bwd"):
            ops.attn_relpos_bwd(x[:, :D], x[:, D:2 * D], x[:, 2 * D:], ek, ek, x[:, :D], x[:, :D], torch.zeros(1, R, dtype=F32, device=dev),
                                dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:], dt[0], dt[1], 1, T, 0.125)
        for buf, n in ((o, "o"), (lse, "lse2"), (dqkv, "dq | dk | dv"), (dt[0], "d_rel_k"), (dt[1], "d_rel_v")):
            untouched(buf, [], f"refused (R {R}, T {T}, P {P}): {n}")


@pytest.mark.parametrize("case", [(256, 16, 2, 16), (264, 8, 1, 4)], ids=lambda c: "x".join(map(str, c)))
def test_attn_relpos_with_zero_tables_matches_attn_small(dev, case):
    """a sanity link to the shipped kernel: with both tables zero, o, lse2, dq, dk, dv agree with attn_small's masked mode on the same
    inputs (bit equality is not required: the two kernels stage their operands differently)"""
    from vt355 import ops
    R, T, H, P = case
    D = H * 64
    z = torch.zeros(2 * P + 1, 64)
    got = _run(dev, case, tables=(z, z))
    d = got["qkv"].view(1, R, 3 * D)
    o = poisoned((1, R, D), BF, dev); lse = poisoned((1, H, R), F32, dev); dqkv = poisoned((1, R, 3 * D), BF, dev)
    ops.attn_small_fwd(d[..., :D], d[..., D:2 * D], d[..., 2 * D:], o, lse, H, 0.125, mask_block=T)
    ops.attn_small_bwd(d[..., :D], d[..., D:2 * D], d[..., 2 * D:], o, got["do"].view(1, R, D), lse,
                       dqkv[..., :D], dqkv[..., D:2 * D], dqkv[..., 2 * D:], H, 0.125, mask_block=T)
    close(got["o"], o[0].float(), 2e-2, 1e-2, "o vs attn_small")
    close(got["lse2"], lse[0], 1e-3, 2e-2, "lse2 vs attn_small")
    close(got["dqkv"], dqkv[0].float(), 3e-2, 2e-2 * dqkv.float().abs().max().item(), "dq | dk | dv vs attn_small")


# ------------------------------------------------------------------------------------------------ the VideoCrafter1 UNet
G_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEPT_TABLES = ("input_blocks.1.2.transformer_blocks.0.attn1.relative_position_k.embeddings_table",
               "middle_block.2.transformer_blocks.0.attn2.relative_position_v.embeddings_table")


def _unet_args(cfg, **kw):
    args = dict(in_channels=cfg.in_channels, out_channels=cfg.out_channels, model_channels=cfg.model_channels,
                attention_resolutions=list(cfg.attention_resolutions), num_res_blocks=cfg.num_res_blocks, channel_mult=list(cfg.channel_mult),
                num_head_channels=64, transformer_depth=1, context_dim=cfg.context_dim, use_linear=True, use_checkpoint=True,
                temporal_conv=False, temporal_attention=True, temporal_selfatt_only=True, use_relative_position=True,
                use_causal_attention=False, temporal_length=cfg.temporal_length, addition_attention=True, fps_cond=True)
    args.update(kw)
    return args


def _vc1_model(dev, seed=17):
    from vt355.unet import UNetModel
    cfg = RR.vc1_tiny_config()
    m = UNetModel(**_unet_args(cfg))
    P = RR.vc1_init_params(cfg, seed=seed)
    assert list(P) == list(m.state_dict()), "parameter names / order differ from the reference's state_dict"
    m.load_state_dict(P)
    m.to(dev)
    m.eval()
    Pr = {k: v.detach().float().cpu().double() for k, v in m.state_dict().items()}       # the bf16-rounded weights the device uses
    return cfg, m, Pr


def _vc1_golden():
    import golden_io
    g = golden_io.load("vc1_unet_tiny")
    return g, {k: torch.from_numpy(g[k]) for k in ("x", "context", "t", "fps", "noise", "out")}


def test_tiny_vc1_unet_forward_matches_golden_and_restatement(dev):
    """forward on the golden inputs of the REFERENCE UNetModel(use_relative_position=True, temporal_conv=False) run: vs the reference
    output (weights differ by bf16 rounding) and vs the restatement on the rounded weights -- test_unet_gpu.py's bars for the tiny VC2 net"""
    from parity import rel_l2
    cfg, m, Pr = _vc1_model(dev)
    g, T = _vc1_golden()
    with torch.no_grad():
        out = m(T["x"].to(dev, BF), T["t"].to(dev), context=T["context"].to(dev, BF), fps=T["fps"].to(dev))
        ref = RR.vc1_unet_forward(Pr, cfg, T["x"].to(BF).double(), T["t"], T["context"].to(BF).double(), fps=T["fps"])
    e_or, e_gold = rel_l2(out, ref), rel_l2(out, T["out"])
    print(f"[vc1 unet tiny fwd] rel-L2 vs restatement {e_or:.3e}, vs reference golden (fp32 weights) {e_gold:.3e}")
    assert e_or < 3e-2 and e_gold < 5e-2


def test_tiny_vc1_unet_train_step_matches_restatement(dev):
    """eps-MSE loss, every parameter gradient (the 32 tables among them) against the fp64 restatement with bars from its bf16 noise floor, the
    kept tables also against the reference module's own gradients, and one AdamW step that moves both kept tables"""
    from parity import bf16_leaves, floor_report, overall_bar, rel_l2
    from vt355 import ops
    from vt355.optim import FusedAdamW
    cfg, m, Pr = _vc1_model(dev)
    ts = m.enable_training()
    g, T = _vc1_golden()
    x, ctx, t, fps, noise = T["x"], T["context"], T["t"], T["fps"], T["noise"]
    out = m(x.to(dev, BF), t.to(dev), context=ctx.to(dev, BF), fps=fps.to(dev))
    loss = poisoned((1,), F32, dev); dp = poisoned(out.shape, BF, dev)
    ops.mse_loss(out.detach().contiguous(), noise.to(dev), loss, dp)
    out.backward(dp)
    for v in Pr.values():
        v.requires_grad_(True)
    ref = RR.vc1_unet_forward(Pr, cfg, x.to(BF).double(), t, ctx.to(BF).double(), fps=fps)
    lref = ((ref - noise.double()) ** 2).mean(dim=(1, 2, 3, 4)).mean()
    lref.backward()
    assert abs(loss.item() - lref.item()) < 2e-2 * lref.item(), (loss.item(), lref.item())
    assert abs(loss.item() - float(g["loss"])) < 5e-2 * float(g["loss"])
    Pb = bf16_leaves(Pr)
    outb = RR.vc1_unet_forward(Pb, cfg, x.to(BF), t, ctx.to(BF), fps=fps)
    assert outb.dtype == BF
    ((outb.float() - noise.float()) ** 2).mean(dim=(1, 2, 3, 4)).mean().backward()
    pairs = [(n, m._view(ts.grad, n).detach().double().cpu(), Pr[n].grad) for n in m.shapes]
    overall, ofloor, worst, bad, ratio, at = floor_report(pairs, {n: Pb[n].grad for n in m.shapes}, 0.98, 0.2)
    kept = {n: rel_l2(m._view(ts.grad, n), torch.from_numpy(g["grad." + n])) for n in KEPT_TABLES}
    print(f"[vc1 unet tiny train] loss dev {loss.item():.6f} restatement {lref.item():.6f} golden {float(g['loss']):.6f}; grads: overall rel-L2 "
          f"{overall:.3e} (bf16 floor {ofloor:.3e}), worst per-parameter {worst:.3e}, worst device / floor {ratio:.2f} at {at}; kept tables vs "
          f"the reference's gradients {kept}")
    assert not bad, bad[:10]
    assert overall < overall_bar(5e-2, ofloor)
    assert all(v < 0.2 for v in kept.values()), kept
    opt = FusedAdamW(ts.params, lr=1e-3, fullft_state=ts)
    before = ts.flat.clone()
    opt.step()
    assert torch.isfinite(ts.flat).all() and torch.equal(ts.flat_bf16.float(), ts.flat.to(BF).float())
    for n in KEPT_TABLES:
        assert (m._view(ts.flat, n) - m._view(before, n)).abs().max().item() > 0, n


def test_tiny_vc1_unet_lora(dev):
    """add_lora() on a relative-position net: with freshly initialised adapters (B = 0) the forward is the no-LoRA forward -- held to the
    forward test's own bar, since two identical calls of this engine already differ through GroupNorm's fp32 atomics
    (test_dc_gpu.py::test_tiny_dc_unet_fs_none_is_default_fs) --, the backward runs with frozen tables, and the adapters get gradients"""
    from parity import rel_l2
    from vt355 import ops
    cfg, m, Pr = _vc1_model(dev)
    g, T = _vc1_golden()
    args = (T["x"].to(dev, BF), T["t"].to(dev))
    kw = dict(context=T["context"].to(dev, BF), fps=T["fps"].to(dev))
    with torch.no_grad():
        plain = m(*args, **kw)
    m.add_lora(4, 1.0, ("to_q", "to_k", "to_v"))
    assert not any(p.requires_grad for n, p in m.named_parameters() if n.endswith(".embeddings_table"))
    ts = m.enable_lora_training()
    assert m.train_state is None
    out = m(*args, **kw)
    e = rel_l2(out, plain)
    print(f"[vc1 unet tiny LoRA] B = 0 forward vs no-LoRA forward rel-L2 {e:.3e}")
    assert e < 3e-2
    loss = poisoned((1,), F32, dev); dp = poisoned(out.shape, BF, dev)
    ops.mse_loss(out.detach().contiguous(), T["noise"].to(dev), loss, dp)
    out.backward(dp)
    assert bool(torch.isfinite(ts.grad).all()) and bool(torch.isfinite(loss).all())
    gb = [m.lora._view(ts.grad, n) for n in m.lora.shapes if ".lora_B." in n and ".2.transformer_blocks." in n]       # temporal blocks
    assert len(gb) and all(float(v.abs().max()) > 0 for v in gb)


def test_vc1_flow_training_step(dev):
    """the vc1 recipe yaml, its UNet shrunk to the tiny size, through vt355.config into LVDMFlow: one training_step with a pinned seed gives
    a finite loss and non-zero gradients in the relative-position tables"""
    import copy
    from vt355.config import instantiate_from_config, load_yaml
    from vt355.lvdm import LVDMFlow
    cfg = RR.vc1_tiny_config()
    node = copy.deepcopy(load_yaml(os.path.join(G_DIR, "vc1_t2v_1024.yaml"))["model"])
    up = node["params"]["unet_config"]["params"]
    assert up["use_relative_position"] is True and up["temporal_conv"] is False
    up.update(model_channels=cfg.model_channels, attention_resolutions=list(cfg.attention_resolutions), num_res_blocks=cfg.num_res_blocks,
              channel_mult=list(cfg.channel_mult), context_dim=cfg.context_dim, temporal_length=cfg.temporal_length)
    flow = instantiate_from_config(node)
    assert type(flow) is LVDMFlow and flow.scale_arr.shape == (1000,)
    flow.model.load_state_dict(RR.vc1_init_params(cfg, seed=17))
    flow.to(dev)
    flow.train()
    flow.model.dropout_seed = 11
    flow.configure_optimizers()
    ts = flow.model.train_state
    torch.manual_seed(1234)
    gen = torch.Generator().manual_seed(5)
    B, T, H, W = 2, cfg.temporal_length, 8, 8
    batch = {"latents": torch.randn(B, 4, T, H, W, generator=gen).to(dev), "context": torch.randn(B, 77, cfg.context_dim, generator=gen).to(dev, BF),
             "fps": torch.tensor([24, 8], device=dev), "null_context": torch.zeros(77, cfg.context_dim, device=dev, dtype=BF)}
    loss = flow.training_step(batch)
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(ts.grad).all())
    m = flow.model
    for n in RR.vc1_table_names(cfg):
        assert float(m._view(ts.grad, n).abs().max()) > 0, n
