"""Gradient clipping on the device (vt_grad_sqnorm -> vt_clip_finalize -> vt_adamw_clip) through the C-ABI: the norm against float64,
the coefficient against torch's formula, the clipped AdamW against torch.optim.AdamW + torch.nn.utils.clip_grad_norm_ / clip_grad_value_,
whole flows against a CPU torch step on the copied gradients, and the DDP ordering."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from grad_clip_common import close, sqnorm_rel_bound, tiny_dc_flow
from parity import poisoned

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")


def _guarded(n, off, dev):
    """n fp32 values whose first element sits ``off`` elements after a 16-byte boundary, inside a buffer of NaNs"""
    buf = torch.full((n + 12,), NAN, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[4 + off:4 + off + n]
    assert v.data_ptr() % 16 == 4 * off
    return buf, v


def _fill(v, mag, seed, spikes=1000):
    g = torch.Generator(device=v.device).manual_seed(seed)
    v.copy_(torch.randn(v.numel(), generator=g, device=v.device) * mag)
    idx = torch.randint(0, v.numel(), (spikes,), generator=g, device=v.device).unique()
    v[idx] *= 1e3


def _ulps(got: float, ref: float) -> float:
    return abs(float(np.float32(got)) - ref) / float(np.spacing(np.float32(ref)))


def _norm_pass(ops, bufs, dev, grad_scale=1.0, max_norm=1.0):
    P = ops.grad_sqnorm_partials()
    partials = torch.full((len(bufs) * P,), NAN, device=dev)
    record = torch.full((2,), NAN, device=dev)
    for s, b in enumerate(bufs):
        ops.grad_sqnorm(b, partials, s)
    ops.clip_finalize(partials, len(bufs), grad_scale, max_norm, record)
    return partials, record


# ------------------------------------------------------------------------------------------------ 4. the norm kernel vs float64
@pytest.mark.parametrize("mag", [1e-3, 1.0])
@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 255, 256 * 1024 + 3, 2 ** 26 + 5])
def test_grad_sqnorm_matches_float64(dev, n, off, mag):
    """Bound, derived (grad_clip_common.sqnorm_rel_bound): (m + t + 1) * 2^-24 on the sum of squares, half of it on the norm, with m the
    per-thread additions of the grid the library reports and t = 10 tree levels.  Checked on the partial sums themselves (summed here in
    float64), so the fp32 rounding of the record is not part of it; the record is then the fp32 rounding of that norm (1 ulp: the order
    of the double additions differs).  NaNs sit right before and after the range: a finite result has not read them."""
    from vt355 import ops
    P = ops.grad_sqnorm_partials()
    assert P == 2048
    buf, v = _guarded(n, off, dev)
    _fill(v, mag, seed=n + 7 * off)
    before = buf.clone()
    ref = math.sqrt((v.double() ** 2).sum().item())
    partials, record = _norm_pass(ops, [v], dev, max_norm=ref / 2)
    assert torch.isfinite(partials).all() and partials.numel() == P
    got = math.sqrt(partials.double().sum().item())
    bound = sqnorm_rel_bound(n, P) / 2
    rel = abs(got - ref) / ref
    print(f"[sqnorm] n {n} off {off} mag {mag:g}: norm {got:.9g} float64 {ref:.9g} rel {rel:.3e} bound {bound:.3e}")
    assert rel <= bound, (rel, bound)
    assert _ulps(record[0].item(), got) <= 1.0
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), "the norm pass wrote to the gradient buffer"
    partials2, record2 = _norm_pass(ops, [v], dev, max_norm=ref / 2)
    assert torch.equal(partials.view(torch.int32), partials2.view(torch.int32)) and torch.equal(record.view(torch.int32), record2.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 5. the coefficient
def test_clip_coefficient_is_torchs_formula(dev):
    from vt355 import ops
    P = ops.grad_sqnorm_partials()
    n = 100003
    _, a = _guarded(n, 1, dev)
    _fill(a, 1e-2, seed=3)
    a.mul_(0.5 / math.sqrt((a.double() ** 2).sum().item()))                     # the recipe's scale: c = 0.5, a norm next to it
    partials, record = _norm_pass(ops, [a], dev)
    tn64 = math.sqrt(partials.double().sum().item())
    assert abs(tn64 - math.sqrt((a.double() ** 2).sum().item())) / tn64 <= sqnorm_rel_bound(n, P) / 2

    def finalize(c, s=1.0):
        rec = torch.full((2,), NAN, device=dev)
        ops.clip_finalize(partials, 1, s, c, rec)
        return rec[0].item(), rec[1].item()

    tn = finalize(1.0)[0]                                                       # the fp32 norm of the record
    assert _ulps(tn, tn64) <= 1.0
    up = float(np.nextafter(np.float32(tn + 1e-6), np.float32(np.inf)))         # the first fp32 c with tn + 1e-6 <= c for certain
    for c in (tn / 20, tn / 1.01, tn, up, 2 * tn, 100.0):                        # norm far above, barely above, at, just below, below c
        c = float(np.float32(c))                                                # what crosses the C-ABI
        total, coef = finalize(c)
        assert total == tn
        want = min(1.0, c / (total + 1e-6))                                     # float64, from the fp32 norm torch would hold
        assert _ulps(coef, want) <= 2.0, (c, coef, want)
        assert (coef == 1.0) == (total + 1e-6 <= c), (c, total, coef)
    assert finalize(tn)[1] < 1.0 and finalize(up)[1] == 1.0
    # grad_scale moves the norm proportionally (the DDP mean, the accumulation mean)
    assert finalize(1.0, 0.25)[0] == 0.25 * tn
    total, coef = finalize(float(np.float32(tn / 6)), 1.0 / 3.0)
    s = float(np.float32(1.0 / 3.0))
    assert _ulps(total, s * tn64) <= 1.0 and _ulps(coef, float(np.float32(tn / 6)) / (total + 1e-6)) <= 2.0
    # two buffers into one array of partial sums: the norm of their concatenation
    _, b = _guarded(777, 3, dev)
    _fill(b, 1.0, seed=4, spikes=10)
    p2, r2 = _norm_pass(ops, [a, b], dev, max_norm=1.0)
    cat = math.sqrt((torch.cat([a, b]).double() ** 2).sum().item())
    got = math.sqrt(p2.double().sum().item())
    assert abs(got - cat) / cat <= sqnorm_rel_bound(n, P) / 2 and _ulps(r2[0].item(), got) <= 1.0
    assert abs(cat - tn64) / cat > 1e-3                                          # ... and not the norm of one of them
    # a non-finite norm gives a non-finite coefficient, as torch (error_if_nonfinite=False)
    b[5] = NAN
    _, r3 = _norm_pass(ops, [a, b], dev)
    assert math.isnan(r3[0].item()) and math.isnan(r3[1].item())


# ------------------------------------------------------------------------------------------------ 6. clipped AdamW vs torch
def _scaled_grads(g, n, c, factors):
    out = []
    for f in factors:
        x = torch.randn(n, generator=g) * 0.1
        out.append((x.double() * (f * c / x.double().norm())).float())
    return out


@pytest.mark.parametrize("algo", ["norm", "value"])
def test_clipped_adamw_matches_torch(dev, algo):
    """the AdamW part of test_noise_loss_adamw (construction and bars) with clipping in front: step 1 clips hard (20 c), step 2 barely
    (1.01 c), step 3 not at all"""
    from vt355 import ops
    g = torch.Generator().manual_seed(5)
    n, c = 5000, 0.5
    p = torch.randn(n, generator=g)
    gr = _scaled_grads(g, n, c, (20.0, 1.01, 0.5)) if algo == "norm" else [torch.randn(n, generator=g) * 0.1 for _ in range(3)]
    cv = 0.05
    pt = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=1e-2)
    P = p.to(dev); Mo = torch.zeros(n, device=dev); Vo = torch.zeros(n, device=dev); Pb = poisoned((n,), BF, dev)
    coefs = []
    for i in range(3):
        pt.grad = gr[i].clone()
        if algo == "norm":
            torch.nn.utils.clip_grad_norm_([pt], c)
        else:
            torch.nn.utils.clip_grad_value_([pt], cv)
        opt.step()
        G = gr[i].to(dev)
        keep = G.clone()
        if algo == "norm":
            _, record = _norm_pass(ops, [G], dev, max_norm=c)
            ops.adamw(P, G, Mo, Vo, Pb, 1e-2, 0.9, 0.999, 1e-8, 1e-2, i + 1, clip_coef=record[1:2])
            coefs.append(record[1].item())
        else:
            ops.adamw(P, G, Mo, Vo, Pb, 1e-2, 0.9, 0.999, 1e-8, 1e-2, i + 1, clip_value=cv)
        assert torch.equal(G.view(torch.int32), keep.view(torch.int32)), "the gradient buffer was rewritten"
    if algo == "norm":
        print(f"[clipped adamw] coefficients {coefs}")
        assert abs(coefs[0] - 0.05) < 1e-5 and abs(coefs[1] - 1 / 1.01) < 1e-5 and coefs[2] == 1.0
    close(P, pt, 1e-5, 1e-6, f"adamw clip {algo}")
    close(Pb, pt, 1e-2, 1e-3, f"adamw clip {algo} bf16 copy")
    # the guard stays first: with the word set nothing moves
    guard = torch.ones(1, dtype=torch.int32, device=dev)
    state = [t.clone() for t in (P, Mo, Vo, Pb)]
    one = torch.full((1,), 0.5, device=dev)
    kw = dict(clip_coef=one) if algo == "norm" else dict(clip_value=cv)
    ops.adamw(P, gr[0].to(dev), Mo, Vo, Pb, 1e-2, 0.9, 0.999, 1e-8, 1e-2, 4, 1.0, guard, **kw)
    for a, b in zip((P, Mo, Vo, Pb), state):
        assert torch.equal(a, b), "vt_adamw_clip ran although the guard was set"
    from vt355._lib import VtError
    with pytest.raises(VtError):                                                 # one algorithm per step
        ops.adamw(P, gr[0].to(dev), Mo, Vo, Pb, 1e-2, 0.9, 0.999, 1e-8, 1e-2, 4, clip_coef=one, clip_value=cv)


def test_clipping_off_is_bit_equal_to_an_optimizer_built_without_it(dev):
    from vt355.optim import FusedAdamW
    g = torch.Generator().manual_seed(11)
    shapes = [(37, 5), (1001,), (64, 64)]
    init = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) * 10 for s in shapes] for _ in range(3)]
    outs = []
    for kw in ({}, dict(gradient_clip_val=None), dict(gradient_clip_val=0, gradient_clip_algorithm="value")):
        ps = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
        opt = FusedAdamW(ps, lr=1e-2, **kw)
        for step in grads:
            for p, x in zip(ps, step):
                p.grad = x.to(dev)
            opt.step(grad_scale=0.5)
        assert opt.grad_norm is None
        outs.append([p.detach().clone() for p in ps] + list(opt.m) + list(opt.v))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 7. whole optimizers / flows
def _two_clipped_steps_vs_torch(opt, masters, grads, copies, lr, c, what):
    """masters / grads: the device buffers the optimizer updates / reads; copies: bf16 compute copies (or None).  Step 1 on the gradients
    as they are (c is chosen so that it clips), step 2 on a quarter of them (it does not): the moments then mix two different
    coefficients, so a wrong one shows in the masters (one AdamW step alone is invariant to the gradient's scale).  Expected = CPU
    torch.optim.AdamW on the copied gradients after ONE clip_grad_norm_ over all of them together; the bars of test 6."""
    ps = [m.detach().cpu().clone().requires_grad_(True) for m in masters]
    ref = torch.optim.AdamW(ps, lr=lr)
    norms = []
    for k in range(2):
        keep = [x.clone() for x in grads]
        for p, x in zip(ps, grads):
            p.grad = x.detach().cpu().clone().view_as(p)
        norms.append(float(torch.nn.utils.clip_grad_norm_(ps, c)))
        ref.step()
        opt.step()
        for x, y in zip(grads, keep):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), what + ": the gradient buffer was rewritten"
        n64 = math.sqrt(sum((x.double() ** 2).sum().item() for x in grads))
        got = opt.grad_norm
        assert got.dim() == 0 and got.is_cuda
        assert abs(got.item() - n64) / n64 <= 2.0 ** -20, (what, k, got.item(), n64)       # bounds of test 4 for these sizes (m <= 4) + the fp32 record
        for x in grads:
            x.mul_(0.25)
    assert norms[0] > c * 1.5 and norms[1] < c, (what, norms, c)
    for i, (m, p) in enumerate(zip(masters, ps)):
        close(m, p, 1e-5, 1e-6, f"{what} master {i}")
    for i, (b, p) in enumerate(zip(copies, ps)):
        if b is not None:
            close(b, p, 1e-2, 1e-3, f"{what} bf16 copy {i}")


def test_dc_flow_clips_the_joint_norm_of_unet_and_resampler(dev):
    """tiny DynamiCrafter flow: one training_step + backward, then clipped steps with gradient_clip_val = half the measured JOINT norm,
    against a CPU torch step on the copied gradients (two backward passes differ in the last bits, GroupNorm's atomics, so no second run
    is compared)"""
    cfg, flow = tiny_dc_flow()
    import dc_oracle as DC
    flow.to(dev)
    flow.train()
    flow.configure_optimizers()
    uts, rts = flow.model.train_state, flow.image_proj_model.train_state
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(17)
    B, T, H, W = 2, cfg.temporal_length, 8, 8
    batch = {"latents": torch.randn(B, 4, T, H, W, generator=g).to(dev), "context": torch.randn(B, 77, cfg.context_dim, generator=g).to(dev, BF),
             "image_tokens": torch.randn(B, 9, DC.RS_FLOW["embedding_dim"], generator=g).to(dev, BF), "fps": torch.tensor([24, 3]).to(dev),
             "null_context": torch.zeros(77, cfg.context_dim, device=dev, dtype=BF),
             "null_image_tokens": torch.zeros(9, DC.RS_FLOW["embedding_dim"], device=dev, dtype=BF)}
    flow.training_step(batch).backward()
    nu = math.sqrt((uts.grad.double() ** 2).sum().item()); nr = math.sqrt((rts.grad.double() ** 2).sum().item())
    joint = math.hypot(nu, nr)
    print(f"[dc clip] |g| UNet {nu:.6g} Resampler {nr:.6g} joint {joint:.6g}")
    assert (joint - nu) / joint > 1e-4 and (joint - nr) / joint > 1e-4, "a per-module norm would pass: the test shows nothing"
    c = joint / 2
    opt = flow.configure_optimizers(gradient_clip_val=c)
    _two_clipped_steps_vs_torch(opt, [uts.flat, rts.flat], [uts.grad, rts.grad], [uts.flat_bf16, rts.flat_bf16], flow.learning_rate, c, "dc flow")
    assert opt.optimizers[1]._clip_partials is None, "the Resampler's optimizer ran a norm pass of its own"
    assert all(o.grad_norm.data_ptr() == opt.grad_norm.data_ptr() for o in opt.optimizers)


def test_cogvideox_lora_step_clips(dev):
    """one tiny CogVideoX LoRA step (flat LoraState) through CogVideoX's loss, then the clipped steps"""
    from selfcheck import build_tiny
    from vt355.optim import FusedAdamW
    from vt355.scheduler import CogVideoXDPMScheduler
    from vt355.workflow import _LossFn
    cfg, model, peft, st = build_tiny(dev)
    g = torch.Generator().manual_seed(123)
    B, Fr = 2, (cfg.sample_frames - 1) // 4 + 1
    x0 = torch.randn(B, Fr, 16, cfg.sample_height, cfg.sample_width, generator=g)
    text = (torch.randn(B, cfg.max_text_seq_length, cfg.text_embed_dim, generator=g) * 0.5).to(BF)
    noise = torch.randn(x0.shape, generator=g)
    t = torch.tensor([200, 800])
    sched = CogVideoXDPMScheduler()
    noisy = sched.add_noise(x0.to(dev), noise.to(dev), t.to(dev))
    out = peft(hidden_states=noisy, encoder_hidden_states=text.to(dev), timestep=t.to(dev), return_dict=False)[0]
    sa, sb, w = sched.coefficients(t.to(dev))
    st.grad.zero_()
    _LossFn.apply(out, noisy, x0.to(dev), sa, sb, w).backward()
    c = math.sqrt((st.grad.double() ** 2).sum().item()) / 2
    assert c > 0
    opt = FusedAdamW(st.params, lr=1e-3, lora_state=st, gradient_clip_val=c)
    _two_clipped_steps_vs_torch(opt, [st.flat], [st.grad], [st.flat_bf16], 1e-3, c, "cogvideox lora")


def test_per_tensor_fallback_clips_over_all_tensors(dev):
    """parameters and gradients that are unaligned views of larger buffers (what the per-tensor path hands to the kernels)"""
    from vt355.optim import FusedAdamW
    g = torch.Generator().manual_seed(23)
    sizes = [1, 255, 4099, 70001]
    store, gstore = torch.zeros(sum(sizes) + 16, device=dev), torch.zeros(sum(sizes) + 16, device=dev)
    ps, o = [], 1
    for i, n in enumerate(sizes):
        p = torch.nn.Parameter(store[o:o + n]); p.data.copy_(torch.randn(n, generator=g))
        p.grad = gstore[o:o + n]; p.grad.copy_(torch.randn(n, generator=g) * (10.0 if i == 0 else 0.05))
        ps.append(p); o += n + 1                                                     # every view starts at another offset mod 16 bytes
    assert len({p.data_ptr() % 16 for p in ps}) > 1
    joint = math.sqrt(sum((p.grad.double() ** 2).sum().item() for p in ps))
    c = joint / 2
    opt = FusedAdamW(ps, lr=1e-2, gradient_clip_val=c)
    _two_clipped_steps_vs_torch(opt, [p.data for p in ps], [p.grad for p in ps], [None] * len(ps), 1e-2, c, "per-tensor")


# ------------------------------------------------------------------------------------------------ 8. DDP ordering
def test_ddp_reduce_then_clipped_step_keeps_ranks_bit_equal(dev):
    """world 2 over gloo on the one card: tests/grad_clip_ddp_helper.py starts its two ranks as fresh interpreters before anything of it
    opens the GPU.  The ranks hold different gradients; after reduce() + clipped step their masters are bit-equal, they derived the same
    coefficient bits, and they match the single-process clipped step on the mean gradient within the bars of test 6."""
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)), "grad_clip_ddp_helper.py")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, helper], env=env, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    r0, r1 = res["ranks"]
    print(f"[ddp clip] {res}")
    assert r0["masters_sha256"] == r1["masters_sha256"] and r0["moments_sha256"] == r1["moments_sha256"]
    assert r0["coef_bits"] == r1["coef_bits"] and r0["norm_bits"] == r1["norm_bits"] and len(r0["coef_bits"]) == 3
    assert r0["local_grads_differ"] and r1["local_grads_differ"]
    assert r0["coefs"][0] < 0.5 and r0["coefs"][2] == 1.0
    for r_ in (r0, r1):
        assert r_["out_of_tol_master"] == 0.0 and r_["out_of_tol_bf16"] == 0.0, r_
