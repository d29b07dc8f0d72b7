"""OpenSora STDiT on the device (vt355.stdit) against the CPU oracle (oracle/stdit_oracle.py, pinned to the imported reference STDiT and to
the reference's loss code by tests/golden/stdit_*.npz) -- BASELINE configs[0], SURVEY 8(a) a14-a15."""
import os

import numpy as np
import pytest
import torch

from parity import bf16_leaves, floor_report, poisoned, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _tiny(dev, cfg=None):
    import stdit_oracle as SO
    from vt355.stdit import STDiT
    cfg = cfg or SO.tiny_config()
    m = STDiT(input_size=cfg.input_size, in_channels=cfg.in_channels, patch_size=cfg.patch_size, hidden_size=cfg.hidden_size, depth=cfg.depth,
              num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, class_dropout_prob=0.0, caption_channels=cfg.caption_channels,
              model_max_length=cfg.model_max_length, space_scale=cfg.space_scale, time_scale=cfg.time_scale)
    P = SO.init_params(cfg, seed=3)
    assert list(P) == [k for k, _ in m.named_parameters()]
    m.load_state_dict(P, strict=False)
    m.to(dev)
    Pr = {k: v.detach().float().cpu().double() for k, v in m.named_parameters()}
    return SO, cfg, m, Pr


def _grads_vs_floor(SO, cfg, m, ts, Pr, x_t, t, y, mask, x0, noise, osch):
    """grad_report of every parameter against the fp64 oracle's gradients (the caller's run), with bars from the oracle's own bf16 noise: the
    same step once more on the CPU with bf16 weights, inputs and activations, the loss taken in fp32 from the bf16-rounded output as on the
    device.  Returns (overall, overall bf16 floor, worst, bad, worst device / floor ratio, its parameter)"""
    Pb = bf16_leaves(Pr)
    outb = SO.stdit_forward(Pb, cfg, x_t.to(BF), t, y.to(BF), mask)
    SO.opensora_loss(outb, x0.float(), noise.float(), t, osch)[0].backward()
    return floor_report([(n, m._view(ts.grad, n), Pr[n].grad) for n in m.shapes], {n: Pb[n].grad for n in m.shapes}, 0.98, 0.2)


def test_tiny_stdit_forward_matches_golden_and_oracle(dev):
    SO, cfg, m, Pr = _tiny(dev)
    g = np.load(os.path.join(G, "stdit_tiny.npz"))
    x, y, mask, t = [torch.from_numpy(g[k]) for k in ("x", "y", "mask", "t")]
    with torch.no_grad():
        out = m(x.to(dev, BF), t.to(dev), y.to(dev, BF), mask.to(dev))
    ref = SO.stdit_forward(Pr, cfg, x.to(BF).double(), t, y.to(BF).double(), mask)
    e1, e2 = rel_l2(out, ref), rel_l2(out, torch.from_numpy(g["out"]))
    print(f"[stdit tiny fwd] rel-L2 vs oracle {e1:.3e}, vs reference golden (fp32 weights) {e2:.3e}")
    assert out.dtype == torch.float32 and e1 < 3e-2 and e2 < 5e-2


def test_tiny_stdit_train_step_matches_oracle(dev):
    """the reference's loss (mse + learned-variance VB term, t = 0 branch included) and every parameter gradient vs the fp64 oracle, each within
    1.5 x the oracle's own bf16 noise.  (These bars found the patch embedding's gradients taken from the last block's output gradient: 15 % off
    on x_embedder.proj.bias, 3.7 x its floor here and 30 x at the recipe's width, inside the old 0.98 / 0.2 bars.)"""
    from vt355 import ops
    from vt355.optim import FusedAdamW
    from vt355.stdit import OpenSoraScheduler, _OpenSoraLoss
    SO, cfg, m, Pr = _tiny(dev)
    ts = m.enable_training()
    gen = torch.Generator().manual_seed(21)
    B = 3
    x0 = torch.randn(B, 4, *cfg.input_size, generator=gen)
    noise = torch.randn(x0.shape, generator=gen)
    y = torch.randn(B, 1, cfg.model_max_length, cfg.caption_channels, generator=gen).to(BF).float()
    mask = torch.zeros(B, cfg.model_max_length, dtype=torch.int64); mask[0, :3] = 1; mask[1, :12] = 1; mask[2, :7] = 1
    t = torch.tensor([0, 250, 999])
    sch = OpenSoraScheduler()
    coef = sch.coef(t.to(dev))
    x_t = poisoned(x0.shape, BF, dev)
    ops.q_sample(x0.to(dev), noise.to(dev), coef[:, 0].float().contiguous(), coef[:, 1].float().contiguous(), None, x_t)
    out = m(x_t, t.to(dev), y.to(dev, BF), mask.to(dev))
    loss = _OpenSoraLoss.apply(out, x0.to(dev), noise.to(dev), coef)
    loss.backward()
    osch = SO.schedule(1000)
    for v in Pr.values():
        v.requires_grad_(True)
    ref = SO.stdit_forward(Pr, cfg, x_t.float().cpu().double(), t, y.double(), mask)
    # the device loss sees the model output rounded through its bf16 rows and cast to fp32, as the reference's fp32 cast does
    lref, mse, vb = SO.opensora_loss(ref.double(), x0.double(), noise.double(), t, {k: (v.double() if v.is_floating_point() else v) for k, v in osch.items()})
    lref.backward()
    print(f"[stdit tiny train] loss dev {loss.item():.5f} oracle {lref.item():.5f} (mse {mse.item():.4f} vb {vb.item():.4f})")
    assert abs(loss.item() - lref.item()) < 2e-2 * abs(lref.item())
    overall, ofloor, worst, bad, ratio, at = _grads_vs_floor(SO, cfg, m, ts, Pr, x_t.float().cpu(), t, y, mask, x0, noise, osch)
    print(f"[stdit tiny train] grads: overall rel-L2 {overall:.3e} (bf16 floor {ofloor:.3e}), worst per-parameter {worst:.3e}, "
          f"worst device / floor {ratio:.2f} at {at}")
    assert not bad, bad[:8]
    assert overall < 1.5 * ofloor, (overall, ofloor)
    opt = FusedAdamW(ts.params, lr=1e-3, fullft_state=ts)
    before = ts.flat.clone()
    opt.step()
    assert torch.isfinite(ts.flat).all() and (ts.flat - before).abs().max().item() > 0


@pytest.mark.parametrize("env", [{"VT355_STDIT_BATCH": "0"}, {"VT355_STDIT_UNPAD": "0"}])
def test_tiny_stdit_batched_paths_equal_the_block_by_block_ones(dev, env, monkeypatch):
    """The per-block small-tensor work is batched over the blocks (head padding of the projections, modulation tables, padded bias
    gradients: VT355_STDIT_BATCH) and the head-padded weight gradients are un-padded inside the GEMM (VT355_STDIT_UNPAD); the block-by-block /
    padded-temporary paths stay as fall-backs.  Same inputs, same weights: output bit-equal, every parameter gradient within fp32
    summation-order noise."""
    from vt355.stdit import _OpenSoraLoss, OpenSoraScheduler
    gen = torch.Generator().manual_seed(5)
    res = []
    for use_env in (False, True):
        for k, v in env.items():
            if use_env:
                monkeypatch.setenv(k, v)
            else:
                monkeypatch.delenv(k, raising=False)
        SO, cfg, m, Pr = _tiny(dev)
        ts = m.enable_training()
        if not res:
            B = 2
            x0 = torch.randn(B, 4, *cfg.input_size, generator=gen).to(dev)
            noise = torch.randn(x0.shape, generator=gen).to(dev)
            y = torch.randn(B, 1, cfg.model_max_length, cfg.caption_channels, generator=gen).to(dev, BF)
            mask = torch.zeros(B, cfg.model_max_length, dtype=torch.int64, device=dev); mask[0, :5] = 1; mask[1, :11] = 1
            t = torch.tensor([3, 700], device=dev)
            coef = OpenSoraScheduler().coef(t)
        out = m(x0.to(BF), t, y, mask)
        _OpenSoraLoss.apply(out, x0, noise, coef).backward()
        res.append((out.detach().clone(), ts.grad.clone()))
    assert torch.equal(res[0][0], res[1][0])
    g0, g1 = res[0][1].double(), res[1][1].double()
    assert (g0 - g1).norm().item() <= 1e-5 * g0.norm().item() and g0.abs().max().item() > 0


def test_stdit_xl2_blocks_at_the_recipes_full_size(dev):
    """Two STDiT-XL/2 blocks at the recipe's real geometry (BASELINE configs[0]): width 1152, 16 heads of 72, 16 x 16 x 16 = 4096 tokens per
    sample, 120 x 4096 T5 captions with a ragged mask -- block 0 carries the temporal position table, block 1 does not.  Forward and every
    parameter gradient against the fp64 oracle; only the depth (2 of 28) is reduced, every kernel runs at its production shape."""
    import stdit_oracle as SO
    from vt355.stdit import _OpenSoraLoss, OpenSoraScheduler
    cfg = SO.STDiTConfig(depth=2)
    assert (cfg.hidden_size, cfg.num_heads, cfg.num_temporal * cfg.num_spatial) == (1152, 16, 4096)
    SO, cfg, m, Pr = _tiny(dev, cfg)
    ts = m.enable_training()
    gen = torch.Generator().manual_seed(5)
    B = 2
    x0 = torch.randn(B, 4, *cfg.input_size, generator=gen)
    noise = torch.randn(x0.shape, generator=gen)
    y = torch.randn(B, 1, cfg.model_max_length, cfg.caption_channels, generator=gen).to(BF).float()
    mask = torch.zeros(B, cfg.model_max_length, dtype=torch.int64); mask[0, :37] = 1; mask[1, :120] = 1
    t = torch.tensor([17, 640])
    coef = OpenSoraScheduler().coef(t.to(dev))
    x_t = (x0 * coef[:, 0].float().cpu().view(B, 1, 1, 1, 1) + noise * coef[:, 1].float().cpu().view(B, 1, 1, 1, 1)).to(BF)
    out = m(x_t.to(dev), t.to(dev), y.to(dev, BF), mask.to(dev))
    loss = _OpenSoraLoss.apply(out, x0.to(dev), noise.to(dev), coef)
    loss.backward()
    torch.cuda.synchronize()
    for v in Pr.values():
        v.requires_grad_(True)
    ref = SO.stdit_forward(Pr, cfg, x_t.double(), t, y.double(), mask)
    e_out = rel_l2(out, ref)
    osch = SO.schedule(1000)
    lref, _, _ = SO.opensora_loss(ref, x0.double(), noise.double(), t, {k: (v.double() if v.is_floating_point() else v) for k, v in osch.items()})
    lref.backward()
    overall, ofloor, worst, bad, ratio, at = _grads_vs_floor(SO, cfg, m, ts, Pr, x_t, t, y, mask, x0, noise, osch)
    print(f"[stdit XL/2 width, depth 2, 2 x 4096 tokens] out rel-L2 {e_out:.3e}; loss dev {loss.item():.5f} oracle {lref.item():.5f}; "
          f"grads overall rel-L2 {overall:.3e} (bf16 floor {ofloor:.3e}), worst per-parameter {worst:.3e}, worst device / floor {ratio:.2f} at {at}")
    assert e_out < 3e-2 and abs(loss.item() - lref.item()) < 2e-2 * abs(lref.item())
    assert not bad, bad[:8]
    assert overall < 1.5 * ofloor, (overall, ofloor)


def test_opensora_loss_kernel_matches_golden(dev):
    """vt_opensora_loss vs the reference's own p_losses run (tests/golden/stdit_loss.npz): loss, mse / vb parts, d loss / d model output"""
    from vt355 import ops
    from vt355.stdit import OpenSoraScheduler
    g = np.load(os.path.join(G, "stdit_loss.npz"))
    T = lambda k: torch.from_numpy(g[k]).to(dev)
    coef = OpenSoraScheduler().coef(T("t"))
    loss3 = poisoned((3,), torch.float64, dev)
    dout = poisoned(g["model_out"].shape, torch.float32, dev)
    ops.opensora_loss(T("model_out"), T("x0"), T("noise"), coef, loss3, dout)
    l = loss3.cpu()
    assert abs(l[0].item() - float(g["loss"])) < 1e-6 * float(g["loss"])
    assert abs(l[1].item() - float(g["loss_mse"])) < 1e-5 * float(g["loss_mse"]) and abs(l[2].item() - float(g["loss_vb"])) < 1e-6 * float(g["loss_vb"])
    r = torch.from_numpy(g["dmodel_out"])
    assert (dout.cpu() - r).abs().max().item() < 1e-4 * r.abs().max().item()


def test_stdit_caption_dropout_follows_the_reference_rule(dev):
    """train mode: CaptionEmbedder.token_drop (opensora/models/layers/blocks.py:783-796) -- `torch.rand(B) < class_dropout_prob` on the CPU
    generator (the reference draws it there and moves it), dropped samples' captions become y_embedding, the mask is left alone.  Compared
    with the oracle fed the captions replaced on the host; `force_drop_ids` forces the same choice in eval mode"""
    SO, cfg, m, Pr = _tiny(dev)
    m.config.class_dropout_prob = 0.5
    gen = torch.Generator().manual_seed(4)
    B = 4
    x = torch.randn(B, 4, *cfg.input_size, generator=gen).to(BF)
    y = torch.randn(B, 1, cfg.model_max_length, cfg.caption_channels, generator=gen).to(BF)
    mask = torch.zeros(B, cfg.model_max_length, dtype=torch.int64); mask[:, :9] = 1
    t = torch.tensor([10, 500, 900, 3])
    torch.manual_seed(11)
    want = torch.rand(B) < 0.5
    assert bool(want.any()) and not bool(want.all())
    ye = m.y_embedder.y_embedding.detach().float().cpu().to(BF)
    y_ref = torch.where(want[:, None, None, None], ye, y)
    m.train()
    torch.manual_seed(11)
    with torch.no_grad():
        out = m(x.to(dev), t.to(dev), y.to(dev), mask.to(dev))
    ref = SO.stdit_forward(Pr, cfg, x.double(), t, y_ref.double(), mask)
    nodrop = SO.stdit_forward(Pr, cfg, x.double(), t, y.double(), mask)
    e = rel_l2(out, ref)
    print(f"[stdit caption dropout] dropped {want.tolist()}; rel-L2 vs oracle with replaced captions {e:.3e}, vs undropped {rel_l2(out, nodrop):.3e}")
    assert e < 3e-2 and rel_l2(out, nodrop) > 10 * e
    m.eval()
    with torch.no_grad():
        out_f = m(x.to(dev), t.to(dev), y.to(dev), mask.to(dev), force_drop_ids=want.to(torch.int64))
        out_e = m(x.to(dev), t.to(dev), y.to(dev), mask.to(dev))
    assert torch.equal(out_f, out) and rel_l2(out_e, nodrop) < 3e-2


def test_whole_stdit_xl2_full_size_backward_predicts_its_own_forward(dev):
    """BASELINE configs[0] at its stated size, one sample: all 28 blocks of STDiT-XL/2 (width 1152, 16 x 72 heads, 16 x 16 x 16 = 4096 tokens,
    120 x 4096 T5 caption with a ragged mask), forward + backward -- beyond what the CPU oracle reaches in a test's time (two blocks are
    checked against it above).  Property: the gradient predicts the forward.  For each of five parameter groups a random subset of the
    weights is moved along the group's own gradient by a few bf16 ulps and  L(w+) - L(w-)  is compared with  <g, w+ - w->  (w+- = the bf16
    weights the kernels read)."""
    import stdit_oracle as SO
    from vt355.stdit import STDiT
    cfg = SO.STDiTConfig()
    m = STDiT(input_size=cfg.input_size, in_channels=cfg.in_channels, patch_size=cfg.patch_size, hidden_size=cfg.hidden_size, depth=cfg.depth,
              num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, class_dropout_prob=0.0, caption_channels=cfg.caption_channels,
              model_max_length=cfg.model_max_length, space_scale=cfg.space_scale, time_scale=cfg.time_scale)
    assert cfg.depth == 28
    m.load_state_dict(SO.init_params(cfg, seed=9), strict=False)
    m.to(dev)
    ts = m.enable_training()
    g = torch.Generator().manual_seed(12)
    x = torch.randn(1, 4, *cfg.input_size, generator=g).to(dev, BF)
    y = torch.randn(1, 1, cfg.model_max_length, cfg.caption_channels, generator=g).to(dev, BF)
    mask = torch.zeros(1, cfg.model_max_length, dtype=torch.int64, device=dev); mask[0, :83] = 1
    t = torch.tensor([321], device=dev)
    r = None

    def fwd():
        return m(x, t, y, mask)

    out = fwd()
    assert torch.isfinite(out).all()
    r = torch.randn(out.shape, generator=g).to(dev)

    def L():
        with torch.no_grad():
            return (fwd().float() * r).sum().item() / r.numel()

    out.backward((r / r.numel()).to(out.dtype))
    torch.cuda.synchronize()
    grad = ts.grad.clone()
    assert torch.isfinite(grad).all()
    groups = {"attn": [], "attn_temp": [], "cross_attn": [], "mlp": [], "rest": []}
    for n, shp in m.shapes.items():
        k = "rest"
        if len(shp) >= 2 and n.startswith("blocks."):
            k = "attn_temp" if ".attn_temp." in n else "cross_attn" if ".cross_attn." in n else "attn" if ".attn." in n else "mlp" if ".mlp." in n else "rest"
        groups[k].append(n)
    assert all(groups.values())
    base = ts.flat_bf16.clone()
    dgen = torch.Generator(device=dev).manual_seed(13)
    L0 = L()
    report = []
    for k, names in groups.items():
        d = torch.zeros_like(grad)
        for n in names:
            gv, wv = m._view(grad, n), m._view(ts.flat, n)
            gn = gv.float().pow(2).mean().sqrt()
            if gn > 0:
                m._view(d, n).copy_(gv * (wv.float().pow(2).mean().sqrt() / gn))
        eps = 0.03
        pred_full = eps * (grad.double() * d.double()).sum().item()
        rho = min(1.0, 2e-3 / max(pred_full, 1e-30))
        d = d * (torch.rand(d.shape, device=dev, generator=dgen) < rho)
        vals = {}
        for sgn in (+1, -1):
            ts.flat_bf16.copy_((ts.flat + sgn * eps * d).to(BF)); ts.version += 1
            vals[sgn] = (L(), ts.flat_bf16.float().clone())
        ts.flat_bf16.copy_(base); ts.version += 1
        measured = vals[+1][0] - vals[-1][0]
        predicted = (grad.double() * (vals[+1][1] - vals[-1][1]).double()).sum().item()
        report.append((k, len(names), measured, predicted))
    print(f"[stdit XL/2 full size, 28 blocks] L0 {L0:.5e}; " + "; ".join(f"{k} ({n} tensors): dL {a:.4e} vs <g, dw> {b:.4e}" for k, n, a, b in report))
    for k, n, a, b in report:
        assert b > 0 and abs(a - b) <= 0.1 * b, (k, a, b)
