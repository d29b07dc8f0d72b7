"""tests/glue_ref.py checked on the CPU: every restatement against the PyTorch call it restates (fp64), the SWEEPS table against the
sources it cites and against the properties the wrap cases rely on, and the single-rounding claims behind the bit-equal bars of
tests/test_glue_kernels_gpu.py."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import glue_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _same(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert bool(((a - b).abs() <= tol * (1.0 + b.abs())).all()), (a - b).abs().max().item()


# ------------------------------------------------------------------ restatements against PyTorch
def test_gelu_restatements_match_torch():
    x = torch.randn(4000, generator=_g(1), dtype=F64) * 3
    _same(R.gelu_erf(x), F.gelu(x))
    _same(R.gelu_tanh(x), F.gelu(x, approximate="tanh"))
    xr = x.clone().requires_grad_(True)
    F.gelu(xr).sum().backward()
    _same(R.gelu_erf_grad(x), xr.grad)


def test_geglu_and_gated_gelu_match_autograd():
    g = _g(2)
    h = torch.randn(13, 48, generator=g, dtype=F64) * 2
    dy = torch.randn(13, 24, generator=g, dtype=F64)
    hr = h.clone().requires_grad_(True)
    a, gate = hr.chunk(2, dim=-1)
    y = a * F.gelu(gate)
    (y * dy).sum().backward()
    _same(R.geglu_fwd(h), y.detach())
    _same(R.geglu_bwd(dy, h), hr.grad)
    _same(R.gated_gelu(h), F.gelu(h[:, :24], approximate="tanh") * h[:, 24:])


@pytest.mark.parametrize("nb,d1,d2", [(2, 3, 5), (1, 1, 4), (3, 4, 1)])
def test_row_maps_match_permute_and_repeat_interleave(nb, d1, d2):
    C = 8
    g = _g(3)
    s = torch.randn(nb, d1, d2, C, generator=g, dtype=F64)
    assert torch.equal(R.row_map(s.view(-1, C), 0, nb, d1, d2).view(nb, d2, d1, C), s.permute(0, 2, 1, 3))
    up = s.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    assert torch.equal(R.row_map(s.view(-1, C), 1, nb, d1, d2).view(up.shape), up)
    z = torch.zeros_like(up); z[:, ::2, ::2] = s
    assert torch.equal(R.row_map(s.view(-1, C), 2, nb, d1, d2).view(up.shape), z)
    big = torch.randn(nb, 2 * d1, 2 * d2, C, generator=g, dtype=F64)
    _same(R.row_map(big.view(-1, C), 3, nb, d1, d2).view(nb, d1, d2, C), big.view(nb, d1, 2, d2, 2, C).sum(dim=(2, 4)))
    # mode 3 is the backward of mode 1
    sr = s.clone().requires_grad_(True)
    (sr.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) * big).sum().backward()
    _same(R.row_map(big.view(-1, C), 3, nb, d1, d2).view(nb, d1, d2, C), sr.grad)


@pytest.mark.parametrize("B,Fr,C,H,W,P", [(2, 3, 5, 4, 6, 2), (1, 2, 3, 8, 4, 4), (2, 1, 4, 3, 5, 1)])
def test_patchify_matches_permute(B, Fr, C, H, W, P):
    img = torch.randn(B, Fr, C, H, W, generator=_g(4), dtype=F64)
    want = img.view(B, Fr, C, H // P, P, W // P, P).permute(0, 1, 3, 5, 2, 4, 6).reshape(B * Fr * (H // P) * (W // P), C * P * P)
    assert torch.equal(R.patchify(img, P), want)
    assert torch.equal(R.unpatchify(want, B, Fr, C, H, W, P), img)
    # (c p q) is the order of a conv2d weight flattened: the patch embedding is a stride-P convolution
    w = torch.randn(7, C, P, P, generator=_g(5), dtype=F64)
    conv = F.conv2d(img.view(B * Fr, C, H, W), w, stride=P).permute(0, 2, 3, 1).reshape(-1, 7)
    _same(R.patchify(img, P) @ w.view(7, -1).t(), conv)


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("shift", [0.0, 1.0])
def test_timestep_embedding_matches_the_written_out_formula(flip, shift):
    t = torch.tensor([0, 1, 17, 999])
    D = 12
    e = R.timestep_embedding(t, D, flip, shift)
    for b in range(4):
        for k in range(D // 2):
            f = math.exp(-math.log(10000.0) * k / (D // 2 - shift))
            s, c = math.sin(t[b].item() * f), math.cos(t[b].item() * f)
            got_s, got_c = (e[b, D // 2 + k], e[b, k]) if flip else (e[b, k], e[b, D // 2 + k])
            assert abs(got_s.item() - s) < 1e-12 and abs(got_c.item() - c) < 1e-12


def test_forward_process_and_losses_match_autograd():
    g = _g(6)
    B = 3
    x0 = torch.randn(B, 2, 3, 4, generator=g, dtype=F64); nz = torch.randn(x0.shape, generator=g, dtype=F64)
    sa = torch.rand(B, generator=g, dtype=F64); sb = (1 - sa * sa).sqrt(); sc = torch.rand(B, generator=g, dtype=F64) + 0.5
    w = torch.rand(B, generator=g, dtype=F64) * 10
    v4 = lambda t: t.view(B, 1, 1, 1)
    _same(R.add_noise(x0, nz, sa, sb), v4(sa) * x0 + v4(sb) * nz)
    _same(R.q_sample(x0, nz, sa, sb, sc), v4(sa * sc) * x0 + v4(sb) * nz)
    _same(R.q_sample(x0, nz, sa, sb, None), R.add_noise(x0, nz, sa, sb))
    noisy = R.add_noise(x0, nz, sa, sb)
    vp = torch.randn(x0.shape, generator=g, dtype=F64).requires_grad_(True)
    loss = R.diffusion_loss(vp, noisy, x0, sa, sb, w)
    want = torch.stack([w[b] * F.mse_loss(sa[b] * noisy[b] - sb[b] * vp[b], x0[b]) for b in range(B)]).mean()
    _same(loss.detach(), want.detach())
    loss.backward()
    grad, terms = R.diffusion_loss_grad(vp.detach(), noisy, x0, sa, sb, w)
    _same(grad, vp.grad)
    assert bool((terms >= grad.abs() * (1 - 1e-12)).all())
    pr = torch.randn(x0.shape, generator=g, dtype=F64).requires_grad_(True)
    l2 = R.mse_loss(pr, nz)
    _same(l2.detach(), F.mse_loss(pr.detach(), nz))
    l2.backward()
    _same(R.mse_loss_grad(pr.detach(), nz)[0], pr.grad)


def test_opensora_loss_matches_the_oracle():
    import stdit_oracle as SO
    g = _g(7)
    B, C = 3, 4
    x0 = torch.randn(B, C, 2, 3, 3, generator=g, dtype=F64).clamp(-1.2, 1.2); x0[0, 0, 0, 0] = torch.tensor([-1.0, 1.0, 0.2], dtype=F64)
    nz = torch.randn(x0.shape, generator=g, dtype=F64)
    out = torch.randn(B, 2 * C, 2, 3, 3, generator=g, dtype=F64) * 0.7
    t = torch.tensor([0, 250, 999])
    sch = {k: (v.double() if v.is_floating_point() else v) for k, v in SO.schedule(1000).items()}
    coef = torch.zeros(B, 8, dtype=F64)
    coef[:, 0] = sch["sqrt_ac"][t]; coef[:, 1] = sch["sqrt_1mac"][t]
    coef[:, 2] = sch["coef1"][t]; coef[:, 3] = sch["coef2"][t]
    coef[:, 4] = sch["posterior_log_variance_clipped"][t]; coef[:, 5] = torch.log(sch["betas"])[t]; coef[:, 6] = (t == 0).double()
    o1 = out.clone().requires_grad_(True); o2 = out.clone().requires_grad_(True)
    mine = R.opensora_loss(o1, x0, nz, coef)
    ref = SO.opensora_loss(o2, x0, nz, t, sch)
    for a, b in zip(mine, ref):
        _same(a.detach(), b.detach(), 1e-10)
    mine[0].backward(); ref[0].backward()
    _same(o1.grad, o2.grad, 1e-10)


def test_adamw_matches_torch_optim_over_five_steps():
    g = _g(8)
    n = 257
    hp = dict(lr=3e-3, betas=(0.95, 0.99), eps=1e-6, weight_decay=0.1)
    p0 = torch.randn(n, generator=g, dtype=F64)
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pt], **hp)
    p, m, v = p0.clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for step in range(1, 6):
        gr = torch.randn(n, generator=g, dtype=F64) * 10.0 ** torch.randint(-9, 1, (n,), generator=g).double()
        pt.grad = gr.clone()
        opt.step()
        p_new, m, v, upd = R.adamw_step(p, gr * 8.0, m, v, hp["lr"], *hp["betas"], hp["eps"], hp["weight_decay"], step, grad_scale=0.125)
        _same(p * (1 - hp["lr"] * hp["weight_decay"]) - upd, p_new, 1e-15)
        p = p_new
        _same(p, pt.detach(), 1e-13)
        st = opt.state[pt]
        _same(m, st["exp_avg"], 1e-13); _same(v, st["exp_avg_sq"], 1e-13)


def test_gate_rows():
    b, txt = R.gate_rows(10, 4, 1)
    assert b.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2] and txt.tolist() == [True, False, False, False] * 2 + [True, False]


# ------------------------------------------------------------------ the SWEEPS table
@pytest.mark.parametrize("row", R.SWEEPS, ids=[r["entry"] for r in R.SWEEPS])
def test_sweeps_rows_wrap_stay_small_and_divide_for_real(row):
    sweep = row["cap"] * 256
    assert row["unit"] in (1, 8)
    assert row["items"] > sweep, "the wrap case does not send any thread round its loop twice"
    assert row["items"] < row.get("max_sweeps", 3) * sweep, "the wrap case is larger than it needs to be"
    assert row.get("max_sweeps", 3) == 3 or row["entry"] == "vt_mse_loss"
    d = row["per_row"]
    assert d > 1 and d & (d - 1) != 0, f"the index split divides by {d}, a power of two: a shift would pass for the division"
    path, line = row["where"].rsplit(":", 1)
    with open(os.path.join(ROOT, path)) as f:
        text = f.read().splitlines()[int(line) - 1]
    assert str(row["cap"]) in text, f"{row['where']} does not state the cap {row['cap']}: {text.strip()}"


def test_sweeps_covers_every_capped_entry_point_once():
    names = [r["entry"] for r in R.SWEEPS]
    assert len(set(names)) == len(names)
    for want in ("vt_geglu_fwd", "vt_geglu_bwd", "vt_gated_gelu_bf16", "vt_add_rows_bf16", "vt_residual_cast_bf16", "vt_dropout_bf16", "vt_gate_mul",
                 "vt_patchify", "vt_unpatchify", "vt_add_noise", "vt_q_sample", "vt_diffusion_loss", "vt_diffusion_loss_bwd", "vt_mse_loss",
                 "vt_opensora_loss", "vt_cast_f32_bf16", "vt_adamw") + tuple(f"vt_row_map_bf16 mode {m}" for m in range(4)):
        assert R.sweep(want)["entry"] == want


# ------------------------------------------------------------------ single rounding behind the bit-equal bars
def _draws(seed, n):
    g = _g(seed)
    return (torch.randn(n, generator=g) * 2.0 ** torch.randint(-12, 13, (n,), generator=g).float()).to(torch.bfloat16)


def test_bf16_sum_through_fp32_rounds_once():
    """add_rows and residual_cast: bf16 + bf16 (or fp32 + bf16) in fp32, then one bf16 store.  2^22 draws over 25 binades: the fp32 sum
    of two bf16 values, rounded to bf16, equals the exact sum rounded once -- so the GPU tests compare bit for bit against fp64."""
    n = 1 << 22
    a, b = _draws(11, n), _draws(12, n)
    got = (a.float() + b.float()).to(torch.bfloat16).double()
    want = R.round_once_bf16(a.double() + b.double())
    assert int((got != want).sum()) == 0


def test_bf16_times_fp32_gate_rounds_once():
    """gate_mul: bf16 x fp32 gate in fp32, then one bf16 store.  With a gate that uses all 24 bits the exact product has up to 32
    significant bits, and the fp32 rounding can land EXACTLY on a bf16 tie that the exact product only came near: 2^22 draws find a few
    dozen such double roundings (47 with these seeds), every one of them a tie of the fp32 product and one bf16 ulp from the
    once-rounded value.  So the GPU test of gate_mul compares bit for bit against the fp32 restatement `(x.float() * g).to(bf16)`,
    not against fp64 rounded once; for a gate that is itself a bf16 value (16 significant bits in the product) the two agree."""
    n = 1 << 22
    x = _draws(13, n)
    g = torch.randn(n, generator=_g(14)) * 2.0 ** torch.randint(-6, 7, (n,), generator=_g(15)).float()
    p32 = x.float() * g
    got = p32.to(torch.bfloat16).double()
    want = R.round_once_bf16(x.double() * g.double())
    bad = got != want
    assert int(bad.sum()) < n // 10000
    assert bool(((p32.view(torch.int32) & 0xFFFF) == 0x8000)[bad].all()), "a mismatch that is not a tie of the fp32 product"
    ulp = 2.0 ** (torch.floor(torch.log2(want.abs()[bad])) - 7)
    assert bool(((got - want).abs()[bad] <= ulp).all())
    gb = g.to(torch.bfloat16).float()
    assert torch.equal((x.float() * gb).to(torch.bfloat16).double(), R.round_once_bf16(x.double() * gb.double()))


def test_round_once_helper_is_bf16_rounding():
    x = torch.randn(100000, generator=_g(16))
    assert torch.equal(R.round_once_bf16(x.double()), x.to(torch.bfloat16).double())      # fp32 -> bf16 is one rounding already
