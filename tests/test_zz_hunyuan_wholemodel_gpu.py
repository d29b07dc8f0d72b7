"""HunyuanVideo denoiser at the shipped recipe's sequence, whole model, LoRA: the backward predicts its own forward (no oracle reaches this
size).  Kept in a file of its own that sorts last: its margin is set by the rounding noise of a bf16 forward, and the driver runs the
suite with -x."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def test_denoiser_at_the_shipped_sequence_lora_backward_predicts_its_own_forward(dev):
    """The shipped recipe's shape (configs/007: 544 x 960 x 17 frames -> latents 16 x 5 x 68 x 120 = 10 200 image tokens + 256 text tokens,
    width 3072, 24 heads of 128) through HunyuanVideoFlow.training_step with a REDUCED DEPTH (3 double + 5 single blocks of 20 + 40: the
    12.8 B-parameter trunk takes minutes to initialise) -- every kernel at its production shape, the embedders, token refiner and final
    layer included.  Property (no oracle reaches this size): the adapter gradient predicts the forward.  For each of four adapter groups a
    random subset of the weights is moved along the group's own gradient by 30 % of its RMS;  L(w+) - L(w-)  must equal  <g, w+ - w->."""
    from vt355.hunyuan import HYVideoDiffusionTransformer, HunyuanVideoFlow
    model = HYVideoDiffusionTransformer(mm_double_blocks_depth=3, mm_single_blocks_depth=5, lora_rank=4).to(dev).init_weights(11)
    model.lora.init_weights(12, zero_b=False)
    flow = HunyuanVideoFlow(model=model, learning_rate=1e-5).to(dev)
    flow.configure_optimizers()
    ts = model.lora.train_state
    g = torch.Generator(device=dev).manual_seed(2)
    Lt = 256
    mask = (torch.arange(Lt, device=dev)[None, :] < 219).long()
    batch = {"latents": torch.randn(1, 16, 5, 68, 120, device=dev, generator=g),
             "prompt_embeds": torch.randn(1, Lt, 4096, device=dev, generator=g).to(BF), "prompt_attention_mask": mask,
             "pooled_prompt_embeds": torch.randn(1, 768, device=dev, generator=g).to(BF)}

    def L():
        torch.manual_seed(4242)                   # training_step draws sigma and the noise
        with torch.no_grad():
            return float(flow.training_step(batch))

    torch.manual_seed(4242)
    loss = flow.training_step(batch)
    ts.grad.zero_(); loss.backward()
    torch.cuda.synchronize()
    grad = ts.grad.clone()
    assert torch.isfinite(grad).all() and grad.abs().max().item() > 0
    L0 = L()
    # the no-grad path draws the same sigma / noise and computes the same loss; the forward is not bit-repeatable (the LoRA down-projection
    # and split-K GEMMs accumulate in fp32 atomics): repeats measured 4e-7 apart, once 1.6e-6; a different draw is off by percents
    assert abs(L0 - loss.item()) <= 1e-5 * abs(L0)
    groups = {"double A": [], "double B": [], "single A": [], "single B": []}
    for n in model.lora.shapes:
        groups[("double" if n.startswith("double_blocks") else "single") + (" A" if ".lora_A" in n else " B")].append(n)
    assert all(groups.values())
    base = model.lora.flat_bf16.clone()
    dgen = torch.Generator(device=dev).manual_seed(14)
    report = []
    for k, names in groups.items():
        d = torch.zeros_like(grad)
        for n in names:
            gv, wv = model.lora._view(grad, n), model.lora._view(ts.flat, n)
            gn = gv.float().pow(2).mean().sqrt()
            if gn > 0:
                model.lora._view(d, n).copy_(gv * (wv.float().pow(2).mean().sqrt() / gn))
        eps = 0.3           # the loss change grows with eps, the bf16 rounding noise of L() does not (eps 0.03: a change of 1.4e-4 of the loss)
        pred_full = eps * (grad.double() * d.double()).sum().item()
        rho = min(1.0, 0.01 * abs(L0) / max(pred_full, 1e-30))
        d = d * (torch.rand(d.shape, device=dev, generator=dgen) < rho)
        vals = {}
        for sgn in (+1, -1):
            model.lora.flat_bf16.copy_((ts.flat + sgn * eps * d).to(BF)); ts.version += 1
            vals[sgn] = (L(), model.lora.flat_bf16.float().clone())
        model.lora.flat_bf16.copy_(base); ts.version += 1
        measured = vals[+1][0] - vals[-1][0]
        predicted = (grad.double() * (vals[+1][1] - vals[-1][1]).double()).sum().item()
        report.append((k, len(names), measured, predicted))
    print(f"[hunyuan 10 456 tokens, 3 + 5 blocks] loss {L0:.5f}; " + "; ".join(f"{k} ({n} tensors): dL {a:.4e} vs <g, dw> {b:.4e}" for k, n, a, b in report))
    # all adapters moved (the subset is everything).  Measured deviation per group against eps, same seeds: 0.03 -> 2-6.5 % (a change of
    # 1.4e-4 of the loss, near the rounding of a bf16 forward; one outlier above 15 % seen), 0.1 -> <= 1.5 %, 0.3 -> <= 1.1 %, 1.0 -> up to
    # 4 % (third-order terms); the forward repeats to 4e-7 of the loss, the gradient to 8e-8.  A wrong gradient (a missing adapter, a lost
    # scaling) is off by factors
    for k, n, a, b in report:
        assert b > 0 and abs(a - b) <= 0.10 * b, (k, a, b)
