"""End-to-end parity of the DiT engine (forward, loss, LoRA gradients, AdamW) against the CPU oracle on seeded tiny
configs, through the public module interface (the same call the reference makes, cogvideo_pl.py:865-871)."""
import pytest
import torch

from parity import bf16_leaves, floor_report, rel_l2

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rope", [False, True], ids=["2b_sincos", "5b_rope"])
def test_tiny_train_step_matches_oracle(dev, rope):
    from selfcheck import tiny_train_step_check
    r = tiny_train_step_check(verbose=True, B=2, rope=rope)
    assert r["cos"] > 0.995


@pytest.mark.parametrize("r", [5, 8, 16])
def test_tiny_train_step_at_higher_lora_ranks(dev, r):
    """peft's LoraConfig (cogvideo_pl.py:143-149) takes any rank; the K-extension's 64 columns hold 3 x r up to r = 16: rank 5 is the last
    one the fused side kernels cover in one call (3 r <= 16), above it each adapter gets its own call on its r columns"""
    from selfcheck import tiny_train_step_check
    out = tiny_train_step_check(verbose=True, B=2, lora_r=r)
    assert out["cos"] > 0.995


def test_forward_no_grad_and_b_zero_init(dev):
    """peft init (B = 0): adapters must not change the forward; dA must be exactly 0 and dB non-zero."""
    import cogvideox_oracle as O
    from selfcheck import build_tiny, oracle_params
    from vt355.scheduler import CogVideoXDPMScheduler
    from vt355.workflow import _LossFn
    cfg, model, peft, st = build_tiny(dev, lora_b_random=False)
    g = torch.Generator().manual_seed(5)
    Fr = (cfg.sample_frames - 1) // 4 + 1
    x0 = torch.randn(1, Fr, 16, cfg.sample_height, cfg.sample_width, generator=g)
    text = (torch.randn(1, cfg.max_text_seq_length, cfg.text_embed_dim, generator=g) * 0.5).to(torch.bfloat16)
    t = torch.tensor([500])
    sched = CogVideoXDPMScheduler()
    noisy = sched.add_noise(x0.to(dev), torch.randn(x0.shape, generator=g).to(dev), t.to(dev))
    with torch.no_grad():
        out_ng = peft(hidden_states=noisy, encoder_hidden_states=text.to(dev), timestep=t.to(dev))[0]
    P, Lo = oracle_params(model, st)
    ref = O.dit_forward(P, cfg, noisy.float().cpu(), text.float(), t, None)
    err = (out_ng.float().cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert err < 5e-2, err
    out = peft(hidden_states=noisy, encoder_hidden_states=text.to(dev), timestep=t.to(dev))[0]
    assert torch.equal(out, out_ng)
    sa, sb, w = sched.coefficients(t.to(dev))
    st.grad.zero_()
    _LossFn.apply(out, noisy, x0.to(dev), sa, sb, w).backward()
    ga = torch.cat([st.view(st.grad, l, k, j).reshape(-1) for (l, k, j) in st._index if k == "A"])
    gb = torch.cat([st.view(st.grad, l, k, j).reshape(-1) for (l, k, j) in st._index if k == "B"])
    assert ga.abs().max().item() == 0.0 and gb.abs().max().item() > 0.0


def test_grad_accumulation_and_state_dict_filter(dev):
    from selfcheck import build_tiny
    from vt355.scheduler import CogVideoXDPMScheduler
    from vt355.workflow import _LossFn
    cfg, model, peft, st = build_tiny(dev)
    g = torch.Generator().manual_seed(9)
    Fr = (cfg.sample_frames - 1) // 4 + 1
    sched = CogVideoXDPMScheduler()

    def one(seed):
        gg = torch.Generator().manual_seed(seed)
        x0 = torch.randn(1, Fr, 16, cfg.sample_height, cfg.sample_width, generator=gg).to(dev)
        text = (torch.randn(1, cfg.max_text_seq_length, cfg.text_embed_dim, generator=gg) * 0.5).to(torch.bfloat16).to(dev)
        t = torch.tensor([300 + seed], device=dev)
        noisy = sched.add_noise(x0, torch.randn(x0.shape, generator=gg).to(dev), t)
        out = peft(hidden_states=noisy, encoder_hidden_states=text, timestep=t)[0]
        sa, sb, w = sched.coefficients(t)
        return _LossFn.apply(out, noisy, x0, sa, sb, w)
    st.grad.zero_(); one(1).backward(); g1 = st.grad.clone()
    st.grad.zero_(); one(2).backward(); g2 = st.grad.clone()
    st.grad.zero_(); (one(1) * 0.5).backward(); (one(2) * 0.5).backward()
    ref = 0.5 * (g1 + g2)
    rel = rel_l2(st.grad, ref)
    assert rel < 2e-2, rel          # fp32 atomics: order-dependent in the last bits only
    # every adapter parameter's .grad aliases the flat buffer
    for p, (l, k, j) in zip(st.params, st._index):
        assert p.grad.data_ptr() == st.view(st.grad, l, k, j).data_ptr()
    sd = peft.state_dict()
    lora_keys = [k for k in sd if "lora" in k]
    assert len(lora_keys) == 2 * 4 * cfg.num_layers and all(k.startswith("base_model.model.") for k in lora_keys)


@pytest.mark.parametrize("variant", ["2b", "5b_rope", "5b_i2v"])
def test_full_finetune_all_parameter_grads_match_oracle(dev, variant):
    """BASELINE config 3 (every weight trainable): loss and ALL parameter gradients of a tiny DiT against the fp64 oracle,
    then one fused AdamW step against torch.optim.AdamW on the oracle's gradients.  Variants: the 2B layout (sincos
    table), the 5B layout (rotary q/k), the 5B-I2V layout (rotary + learned table buffer + 32 input channels)."""
    import cogvideox_oracle as O
    from vt355.dit import CogVideoXTransformer3DModel
    from vt355.fullft import enable_full_finetune
    from vt355.optim import FusedAdamW
    from vt355.scheduler import CogVideoXDPMScheduler
    from vt355.workflow import _LossFn
    from selfcheck import CFG_KEYS
    rope, i2v = variant != "2b", variant == "5b_i2v"
    cfg = O.tiny_config(use_rotary_positional_embeddings=rope, use_learned_positional_embeddings=i2v,
                        in_channels=32 if i2v else 16)
    model = CogVideoXTransformer3DModel(**{k: getattr(cfg, k) for k in CFG_KEYS}).init_weights(11, std=0.05)
    if i2v:         # a checkpointed table differs from the sincos init, text slots included
        gpe = torch.Generator().manual_seed(5)
        model.patch_embed.pos_embedding.copy_((torch.randn(model.patch_embed.pos_embedding.shape, generator=gpe) * 0.1)
                                              .to(torch.bfloat16))
    model = model.to(dev)
    ft = enable_full_finetune(model)
    assert all(p.requires_grad for p in model.parameters())
    g = torch.Generator().manual_seed(77)
    B, Fr = 2, (cfg.sample_frames - 1) // 4 + 1
    x0 = torch.randn(B, Fr, 16, cfg.sample_height, cfg.sample_width, generator=g)
    text = (torch.randn(B, cfg.max_text_seq_length, cfg.text_embed_dim, generator=g) * 0.5).to(torch.bfloat16)
    noise = torch.randn(x0.shape, generator=g)
    t = torch.tensor([150, 650])
    sched = CogVideoXDPMScheduler()
    noisy = sched.add_noise(x0.to(dev), noise.to(dev), t.to(dev))
    model_in = noisy
    if i2v:
        img = torch.zeros(x0.shape)
        img[:, 0] = torch.randn(x0[:, 0].shape, generator=g)
        model_in = torch.cat([noisy, img.to(dev, torch.bfloat16)], dim=2)
    tabs = None
    if rope:
        grid = (cfg.sample_height // 2, cfg.sample_width // 2)
        tabs = O.rope_3d_tables(64, O.resize_crop_region_for_grid(grid, (3, 4)), grid, Fr)
    fwd = lambda: model(hidden_states=model_in, encoder_hidden_states=text.to(dev), timestep=t.to(dev),
                        image_rotary_emb=None if tabs is None else (tabs[0].to(dev), tabs[1].to(dev)))[0]
    out = fwd()
    sa, sb, w = sched.coefficients(t.to(dev))
    loss = _LossFn.apply(out, noisy, x0.to(dev), sa, sb, w)
    ft.grad.zero_()
    loss.backward()
    # oracle on the same bf16-rounded weights, fp64
    Pref = {k: v.detach().float().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    abar = O.alphas_cumprod_cogvideox()
    nref = noisy.float().cpu().double()
    out_ref = O.dit_forward(Pref, cfg, model_in.float().cpu().double(), text.double(), t,
                            image_rotary_emb=None if tabs is None else (tabs[0].double(), tabs[1].double()))
    pred = O.get_velocity(out_ref, nref, t, abar)
    wref = (1.0 / (1.0 - abar[t])).view(-1, 1, 1, 1, 1)
    loss_ref = torch.mean((wref * (pred - x0.double()) ** 2).reshape(B, -1), dim=1).mean()
    loss_ref.backward()
    assert abs(loss.item() - loss_ref.item()) / abs(loss_ref.item()) < 2e-2
    zero_grad = [n for n in ft.names if n.endswith("norm_k.bias") and not rope]
    for name in zero_grad:
        # adding a constant to every key shifts all scores of a query equally: softmax is invariant and the exact
        # gradient is 0 (the oracle returns fp64 noise) -> the device value must be noise-sized, not "aligned"
        assert Pref[name].grad.norm() < 1e-9
        assert ft.g(name).cpu().double().norm() < 0.05 * ft.g(name.replace("bias", "weight")).norm().item(), name
    # the oracle once more in bf16 (same rounded weights and inputs, every op rounding to bf16, the loss in fp32 from the bf16 output): its own
    # distance from fp64 per parameter sets the bars, the old flat 0.15 stays as the cap
    Pb = bf16_leaves(Pref)
    out_b = O.dit_forward(Pb, cfg, model_in.detach().cpu().to(torch.bfloat16), text, t, image_rotary_emb=tabs)
    assert out_b.dtype == torch.bfloat16
    pred_b = O.get_velocity(out_b.float(), nref.float(), t, abar)
    torch.mean((wref.float() * (pred_b - x0) ** 2).reshape(B, -1), dim=1).mean().backward()
    checked = [n for n in ft.names if n not in zero_grad]
    overall, ofloor, worst, bad, ratio, at = floor_report([(n, ft.g(n), Pref[n].grad) for n in checked], {n: Pb[n].grad for n in checked}, 0.99, 0.15)
    print(f"[full fine-tune {variant}] parameter gradients overall rel-L2 {overall:.3e} (bf16 floor {ofloor:.3e}), worst {worst:.3e}, "
          f"worst device / floor {ratio:.2f} at {at}")
    assert not bad, bad[:12]
    assert overall < 1.5 * ofloor, (overall, ofloor)
    # whole-gradient agreement
    gd = ft.grad.cpu().double()
    gr = torch.cat([Pref[n].grad.reshape(-1) for n in ft.names])
    assert torch.nn.functional.cosine_similarity(gd, gr, dim=0).item() > 0.999, torch.nn.functional.cosine_similarity(gd, gr, dim=0).item()
    # optimizer: fused AdamW over the flat fp32 master == torch.optim.AdamW fed the SAME (device) gradients
    master = ft.flat.clone().cpu()
    pt = master.clone().requires_grad_(True)
    topt = torch.optim.AdamW([pt], lr=1e-3)
    pt.grad = ft.grad.clone().cpu()
    topt.step()
    opt = FusedAdamW(ft.params, lr=1e-3, fullft_state=ft)
    v0 = ft.version
    opt.step()
    assert ft.version == v0 + 1
    assert (ft.flat.cpu() - pt.detach()).abs().max().item() < 1e-5
    assert (ft.flat_bf16.float().cpu() - pt.detach()).abs().max().item() < 2e-2 * pt.detach().abs().max().item()
    # the packed transposed operands follow the new weights at the next forward
    out2 = fwd()
    assert torch.isfinite(out2.float()).all() and not torch.equal(out2, out)


def test_encoder_prefetcher_overlaps_on_a_side_stream(dev):
    """SURVEY 8(f) rank 1 plumbing: stand-in 'frozen encoders' (a few matmuls) run on the prefetcher's side stream while the
    main stream is busy; every batch arrives complete, in order, and identical to encoding it synchronously."""
    from vt355.prefetch import EncoderPrefetcher
    g = torch.Generator().manual_seed(3)
    w1 = torch.randn(512, 512, generator=g).to(dev)
    raws = [{"video": torch.randn(4, 512, 512, generator=g), "i": i} for i in range(6)]

    def encode(raw):
        x = raw["video"].to(dev, non_blocking=True)
        for _ in range(8):
            x = torch.tanh(x @ w1 * 0.05)
        return {"latents": x, "prompt_embeds": x.sum(dim=-1), "i": raw["i"]}
    with torch.no_grad():
        want = [encode(r)["latents"].clone() for r in raws]
    torch.cuda.synchronize()
    busy = torch.randn(4096, 4096, device=dev)
    pf = EncoderPrefetcher(raws, encode, device=dev, depth=2)
    assert pf.side is not None and pf.side != torch.cuda.current_stream(dev)
    for k, b in enumerate(pf):
        busy = busy @ busy * 1e-3                   # main-stream work the side stream overlaps with
        assert b["i"] == k
        assert torch.equal(b["latents"], want[k])   # consumed on the main stream after the event wait
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", ["lora", "fullft"])
def test_block_recompute_gives_the_same_gradients(dev, mode):
    """enable_gradient_checkpointing("always") (the reference's policy, cogvideo_pl.py:141) rebuilds every
    block's activations from its input in the backward pass: same loss bit for bit, same gradients up to the order of the
    fp32 atomic adds."""
    import cogvideox_oracle as O
    from vt355.dit import CogVideoXTransformer3DModel
    from vt355.fullft import enable_full_finetune
    from vt355.scheduler import CogVideoXDPMScheduler
    from selfcheck import CFG_KEYS, build_tiny
    from vt355.workflow import _LossFn
    if mode == "lora":
        cfg, model, peft, st = build_tiny(dev)
        call, grad = peft, st.grad
    else:
        cfg = O.tiny_config()
        model = CogVideoXTransformer3DModel(**{k: getattr(cfg, k) for k in CFG_KEYS}).init_weights(11, std=0.05).to(dev)
        ft = enable_full_finetune(model)
        call, grad = model, ft.grad
    g = torch.Generator().manual_seed(3)
    Fr = (cfg.sample_frames - 1) // 4 + 1
    x0 = torch.randn(2, Fr, 16, cfg.sample_height, cfg.sample_width, generator=g).to(dev)
    text = (torch.randn(2, cfg.max_text_seq_length, cfg.text_embed_dim, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    t = torch.tensor([120, 870], device=dev)
    sched = CogVideoXDPMScheduler()
    noisy = sched.add_noise(x0, torch.randn(x0.shape, generator=g).to(dev), t)
    sa, sb, w = sched.coefficients(t)

    def step(policy):
        model.enable_gradient_checkpointing(policy)
        grad.zero_()
        out = call(hidden_states=noisy, encoder_hidden_states=text, timestep=t)[0]
        loss = _LossFn.apply(out, noisy, x0, sa, sb, w)
        loss.backward()
        return loss.item(), grad.clone()
    l0, g0 = step("never")
    l1, g1 = step("always")
    assert l0 == l1
    assert g0.abs().max().item() > 0
    rel = rel_l2(g1, g0)
    assert rel < 1e-3, rel
    with pytest.raises(ValueError):
        model.enable_gradient_checkpointing("sometimes")


@pytest.mark.parametrize("S", [150, 226])
def test_t5_encoder_matches_oracle(dev, S):
    """The frozen text encoder on the vt355 kernels (rmsnorm, fused QKV / wi GEMMs, attention with the relative position
    bias, gated GELU) against oracle/t5_oracle.py -- itself pinned to transformers' T5EncoderModel by tests/golden/t5_tiny.part*.npz.
    bf16 storage vs the fp64 oracle on the bf16-rounded weights."""
    import t5_oracle as T
    from vt355.t5 import T5EncoderModel
    cfg = T.tiny_config(num_layers=3, num_heads=4, d_model=256, d_ff=512)
    m = T5EncoderModel(**vars(cfg)).init_weights(7).to(dev)
    P = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(S)
    ids = torch.randint(0, cfg.vocab_size, (2, S), generator=g)
    out = m(ids.to(dev))
    assert out[0] is out.last_hidden_state and tuple(out[0].shape) == (2, S, cfg.d_model)
    ref = T.encoder_forward(P, cfg, ids)
    err = (out[0].double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert err < 3e-2, err
    cos = torch.nn.functional.cosine_similarity(out[0].double().cpu().reshape(-1), ref.reshape(-1), dim=0).item()
    assert cos > 0.9995, cos


def test_lora_loss_curve_tracks_the_oracle_over_optimizer_steps(dev):
    """North-star parity item "loss curve on fixed seeds": ten optimizer steps of the tiny LoRA recipe (two micro-batches per
    step, AdamW with the reference's defaults, cogvideo_pl.py:774-779) on the device engine -- bf16 activations, fp32 master
    weights, fused AdamW -- against the fp64 oracle trained with torch.optim.AdamW from the same initial adapters (the oracle
    also forwards with the bf16-rounded copy of its master weights, as the device does).  The two loss curves must stay
    together step by step, and training must actually reduce the loss."""
    import cogvideox_oracle as O
    from vt355.optim import FusedAdamW
    from vt355.scheduler import CogVideoXDPMScheduler
    from selfcheck import build_tiny, oracle_params
    from vt355.workflow import _LossFn
    cfg, model, peft, st = build_tiny(dev)
    Fr = (cfg.sample_frames - 1) // 4 + 1
    sched = CogVideoXDPMScheduler()
    abar = O.alphas_cumprod_cogvideox()
    lr, steps, accum, B = 2e-2, 10, 2, 2

    def batch(i):                    # two fixed micro-batches, revisited every step (a curve that can go down)
        g = torch.Generator().manual_seed(1000 + i % accum)
        x0 = torch.randn(B, Fr, 16, cfg.sample_height, cfg.sample_width, generator=g)
        text = (torch.randn(B, cfg.max_text_seq_length, cfg.text_embed_dim, generator=g) * 0.5).to(torch.bfloat16)
        noise = torch.randn(x0.shape, generator=g)
        t = torch.tensor([150 + 40 * (i % accum), 700 - 60 * (i % accum)])
        return x0, text, noise, t

    P, _ = oracle_params(model, st, torch.float64)
    names = []
    for (layer, kind, j) in st._index:
        names.append(f"transformer_blocks.{layer}.attn1.{('to_q', 'to_k', 'to_v', 'to_out.0')[j]}.lora_{kind}.default.weight")
    master = [p.detach().double().cpu().clone().requires_grad_(True) for p in st.params]       # fp32 master values, exactly
    opt_ref = torch.optim.AdamW(master, lr=lr)
    opt_dev = FusedAdamW(st.params, lr=lr, lora_state=st)
    curve_dev, curve_ref = [], []
    for s in range(steps):
        opt_dev.zero_grad(); opt_ref.zero_grad()
        ld = lr_ = 0.0
        for mb in range(accum):
            x0, text, noise, t = batch(mb)
            noisy = sched.add_noise(x0.to(dev), noise.to(dev), t.to(dev))
            out = peft(hidden_states=noisy, encoder_hidden_states=text.to(dev), timestep=t.to(dev), return_dict=False)[0]
            sa, sb, w = sched.coefficients(t.to(dev))
            loss = _LossFn.apply(out, noisy, x0.to(dev), sa, sb, w)
            (loss / accum).backward()
            ld += loss.item() / accum
            # oracle: forward with the bf16-rounded adapters (straight-through to the fp64 master)
            Lo = {n: (m.detach().to(torch.bfloat16).double() - m.detach()) + m for n, m in zip(names, master)}
            noisy_ref = noisy.float().cpu().double()
            out_ref = O.dit_forward(P, cfg, noisy_ref, text.double(), t, Lo, st.scaling)
            pred = O.get_velocity(out_ref, noisy_ref, t, abar)
            wref = (1.0 / (1.0 - abar[t])).view(-1, 1, 1, 1, 1)
            loss_ref = torch.mean((wref * (pred - x0.double()) ** 2).reshape(B, -1), dim=1).mean()
            (loss_ref / accum).backward()
            lr_ += loss_ref.item() / accum
        opt_dev.step(); opt_ref.step()
        curve_dev.append(ld); curve_ref.append(lr_)
    print("loss curve dev", ["%.5f" % v for v in curve_dev]); print("loss curve ref", ["%.5f" % v for v in curve_ref])
    for a, b in zip(curve_dev, curve_ref):
        assert abs(a - b) / b < 1e-3, (curve_dev, curve_ref)          # north_star: "loss curve within 1e-3 ... on fixed seeds"
    assert curve_ref[-1] < 0.99 * curve_ref[0] and curve_dev[-1] < 0.99 * curve_dev[0], (curve_dev, curve_ref)
    drift = torch.cat([p.detach().double().cpu().reshape(-1) - m.detach().reshape(-1) for p, m in zip(st.params, master)])
    moved = torch.cat([m.detach().reshape(-1) for m in master]).norm().item()
    assert drift.norm().item() < 0.1 * moved, (drift.norm().item(), moved)


def test_full_finetune_loss_curve_tracks_the_oracle(dev):
    """Config 3 (every weight trainable): eight optimizer steps of a tiny DiT on the device (bf16 compute copy of the fp32
    master, fused AdamW) against the fp64 oracle trained with torch.optim.AdamW from the same master weights, forwarding with
    their bf16-rounded copy as the device does.  Per-step loss within 1e-3."""
    import cogvideox_oracle as O
    from vt355.dit import CogVideoXTransformer3DModel
    from vt355.fullft import enable_full_finetune
    from vt355.optim import FusedAdamW
    from vt355.scheduler import CogVideoXDPMScheduler
    from selfcheck import CFG_KEYS
    from vt355.workflow import _LossFn
    cfg = O.tiny_config()
    model = CogVideoXTransformer3DModel(**{k: getattr(cfg, k) for k in CFG_KEYS}).init_weights(11, std=0.05).to(dev)
    ft = enable_full_finetune(model)
    lr, steps, B = 2e-4, 8, 2
    Fr = (cfg.sample_frames - 1) // 4 + 1
    sched = CogVideoXDPMScheduler()
    abar = O.alphas_cumprod_cogvideox()
    master = {n: ft.view(ft.flat, n).detach().double().cpu().clone().requires_grad_(True) for n in ft.names}
    opt_ref = torch.optim.AdamW(list(master.values()), lr=lr)
    opt_dev = FusedAdamW(ft.params, lr=lr, fullft_state=ft)
    g = torch.Generator().manual_seed(21)
    x0 = torch.randn(B, Fr, 16, cfg.sample_height, cfg.sample_width, generator=g)
    text = (torch.randn(B, cfg.max_text_seq_length, cfg.text_embed_dim, generator=g) * 0.5).to(torch.bfloat16)
    noise = torch.randn(x0.shape, generator=g)
    t = torch.tensor([250, 720])
    noisy = sched.add_noise(x0.to(dev), noise.to(dev), t.to(dev))
    sa, sb, w = sched.coefficients(t.to(dev))
    nref = noisy.float().cpu().double()
    wref = (1.0 / (1.0 - abar[t])).view(-1, 1, 1, 1, 1)
    extra = {k: v.detach().float().cpu().double() for k, v in model.state_dict().items() if k not in master}      # buffers
    cd, cr = [], []
    for s in range(steps):
        opt_dev.zero_grad(); opt_ref.zero_grad()
        out = model(hidden_states=noisy, encoder_hidden_states=text.to(dev), timestep=t.to(dev))[0]
        loss = _LossFn.apply(out, noisy, x0.to(dev), sa, sb, w)
        loss.backward()
        Pr = {n: (m.detach().to(torch.bfloat16).double() - m.detach()) + m for n, m in master.items()}
        Pr.update(extra)
        out_ref = O.dit_forward(Pr, cfg, nref, text.double(), t)
        pred = O.get_velocity(out_ref, nref, t, abar)
        loss_ref = torch.mean((wref * (pred - x0.double()) ** 2).reshape(B, -1), dim=1).mean()
        loss_ref.backward()
        opt_dev.step(); opt_ref.step()
        cd.append(loss.item()); cr.append(loss_ref.item())
    print("full-FT loss curve dev", ["%.5f" % v for v in cd]); print("full-FT loss curve ref", ["%.5f" % v for v in cr])
    for a, b in zip(cd, cr):
        assert abs(a - b) / b < 1e-3, (cd, cr)
    assert cr[-1] < 0.99 * cr[0] and cd[-1] < 0.99 * cd[0], (cd, cr)


def test_vae_encoder_frame_batches_match_oracle_and_are_causal(dev):
    """num_sample_frames_batch_size=8 (diffusers' frame batching: GroupNorm statistics per frame batch, 9 frames first) on a tiny encoder:
    against the oracle's statement of the same rule, and the property that makes it checkable without diffusers -- the first frame
    batch does not see the later ones: moments of the clip's first 9 frames == the first 3 latent frames of the 25-frame clip"""
    import vae_oracle as V
    from vt355.vae import CogVideoXVaeEncoder
    cfg = V.tiny_config(ch=64)
    m = CogVideoXVaeEncoder(ch=cfg.ch, ch_mult=cfg.ch_mult, num_res_blocks=cfg.num_res_blocks, z_channels=cfg.z_channels,
                            temporal_compress_times=cfg.temporal_compress_times, num_sample_frames_batch_size=8).init_weights(3).to(dev)
    P = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    x = torch.randn(1, 3, 25, 16, 24, generator=torch.Generator().manual_seed(2)).clamp(-1, 1).to(torch.bfloat16)
    out = m(x.to(dev)).float().cpu()
    ref = V.encoder_forward(P, cfg, x.float(), frame_batch=8)
    whole = V.encoder_forward(P, cfg, x.float())
    err = (out - ref).abs().max().item() / ref.abs().max().item()
    assert err < 4e-2 and (ref - whole).abs().max().item() > 10 * (out - ref).abs().max().item()      # the two rules really differ
    head = m(x[:, :, :9].to(dev)).float().cpu()
    assert (head - out[:, :, :3]).abs().max().item() <= 1e-2 * out.abs().max().item()     # same statistics; GroupNorm's atomic sums move last bits


def test_vae_encoder_49_frames_full_resolution_is_causal(dev):
    """one 49x480x720 clip with frame batching: the first 9-frame window's moments equal the full clip's first 3 latent frames"""
    from vt355.vae import CogVideoXVaeEncoder
    m = CogVideoXVaeEncoder(num_sample_frames_batch_size=8).init_weights(1).to(dev)
    x = torch.randn(1, 3, 49, 480, 720, generator=torch.Generator().manual_seed(4)).clamp(-1, 1).to(torch.bfloat16)
    full = m(x.to(dev))
    assert tuple(full.shape) == (1, 32, 13, 60, 90) and torch.isfinite(full.float()).all()
    head = m(x[:, :, :9].to(dev))
    d = (head.float() - full[:, :, :3].float()).abs().max().item()
    print(f"[vae 49x480x720] first window vs full clip: max abs diff {d:.3e} (|moments| max {full.float().abs().max().item():.3f})")
    assert d <= 2e-2 * full.float().abs().max().item()     # GroupNorm sums are atomic: the last bits depend on the launch shape


@pytest.mark.parametrize("T,H,W", [(9, 16, 24), (1, 8, 12), (5, 24, 20)])
def test_vae_encoder_matches_oracle(dev, T, H, W):
    """The CogVideoX VAE encoder on the vt355 kernels (channels-last implicit-GEMM causal convolutions, GroupNorm+SiLU, temporal pool,
    stride-2 downsample, 1x1x1 shortcut GEMM) against oracle/vae_oracle.py -- itself pinned bit for bit to the reference's in-tree
    ContextParallelEncoder3D.  bf16 activations vs the fp32 oracle on the bf16-rounded weights; a single frame (image) too."""
    import vae_oracle as V
    from vt355.vae import CogVideoXVaeEncoder
    cfg = V.tiny_config(ch=64)
    m = CogVideoXVaeEncoder(ch=cfg.ch, ch_mult=cfg.ch_mult, num_res_blocks=cfg.num_res_blocks, z_channels=cfg.z_channels,
                            temporal_compress_times=cfg.temporal_compress_times).init_weights(3).to(dev)
    P = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(T * H)
    x = torch.randn(2, 3, T, H, W, generator=g).clamp(-1, 1).to(torch.bfloat16)
    out = m(x.to(dev))
    ref = V.encoder_forward(P, cfg, x.float())
    assert tuple(out.shape) == tuple(ref.shape)
    err = (out.float().cpu() - ref).abs().max().item() / ref.abs().max().item()
    cos = torch.nn.functional.cosine_similarity(out.float().cpu().reshape(-1), ref.reshape(-1), dim=0).item()
    assert err < 4e-2 and cos > 0.999, (err, cos)
    lat = m.encode(x.to(dev)).latent_dist.sample() * m.config.scaling_factor
    assert tuple(lat.shape) == (2, cfg.z_channels) + tuple(ref.shape[2:]) and torch.isfinite(lat).all()
    gen = torch.Generator(device=dev).manual_seed(5)
    eps = torch.randn(ref[:1, :cfg.z_channels].shape, generator=torch.Generator(device=dev).manual_seed(5), device=dev)
    one = m.latents(x[0].to(dev), generator=gen)                     # the workflow's first_stage callable: one clip [3,T,H,W]
    want = V.sample_latent(out[:1].float(), eps, m.config.scaling_factor)
    assert torch.allclose(one, want, rtol=3e-2, atol=3e-2)           # B=1 vs B=2 launch: GroupNorm's atomic sums differ in the last bits


def test_training_step_from_raw_batch_through_both_encoders(dev):
    """The reference's whole step on the device: a raw {"video", "caption"} batch -> CogVideoX VAE encoder (per clip, sample *
    scaling_factor) + T5 text encoder -> add_noise -> DiT -> loss -> LoRA gradients (cogvideo_pl.py:792-887), with the encoders
    handed to the workflow as first_stage / cond_stage and, a second time, run one batch ahead by EncoderPrefetcher.  The loss must
    equal the one obtained from the same encodings fed as a pre-encoded batch under the same RNG state."""
    import cogvideox_oracle as O
    from vt355.lora import LoraConfig
    from vt355.prefetch import EncoderPrefetcher
    from selfcheck import CFG_KEYS
    from vt355.t5 import FrozenT5Embedder, T5EncoderModel
    from vt355.vae import CogVideoXVaeEncoder
    from vt355.workflow import CogVideoXWorkFlow
    cfg = O.tiny_config()
    enc = CogVideoXVaeEncoder(ch=64, ch_mult=(1, 2, 2), num_res_blocks=1, z_channels=16, temporal_compress_times=4).init_weights(1).to(dev)
    t5 = T5EncoderModel(vocab_size=50, d_model=cfg.text_embed_dim, d_kv=64, d_ff=128, num_layers=2, num_heads=2).init_weights(2).to(dev)
    tok = lambda text, **kw: {"input_ids": torch.tensor([[(ord(ch) * 7 + i) % 50 for i, ch in enumerate(s.ljust(kw["max_length"]))][:kw["max_length"]]
                                                          for s in text])}
    emb = FrozenT5Embedder(tokenizer=tok, transformer=t5, device=dev, max_length=cfg.max_text_seq_length)
    gen = torch.Generator(device=dev)
    wf = CogVideoXWorkFlow(denoiser_config={"target": "vt355.dit.CogVideoXTransformer3DModel", "params": {k: getattr(cfg, k) for k in CFG_KEYS}},
                           scheduler_config={"target": "vt355.scheduler.CogVideoXDPMScheduler"},
                           adapter_config=LoraConfig(r=4, lora_alpha=1.0, target_modules=["to_k", "to_q", "to_v", "to_out.0"]),
                           first_stage=lambda v: enc.latents(v, generator=gen), cond_stage=emb)
    wf.model.base_model.model.init_weights(3)        # the module allocates its weights uninitialised (they come from a checkpoint)
    wf = wf.to(dev)
    st = wf.model._lora_state
    with torch.no_grad():               # peft's B = 0 init hides the adapters: randomise so that every gradient is exercised
        for p, (layer, kind, j) in zip(st.params, st._index):
            if kind == "B":
                p.normal_(0.0, 0.02)
    st.mark_changed()
    g = torch.Generator().manual_seed(8)
    clips = [torch.randn(3, 5, 24, 32, generator=g).clamp(-1, 1).to(dev) for _ in range(2)]      # 5 frames, 24x32 -> latents [16, 2, 6, 8]
    batch = {"video": clips, "caption": ["a red kite over the sea", "two cats"]}
    gen.manual_seed(11); torch.manual_seed(5)
    st.grad.zero_()
    loss = wf.training_step(batch)
    loss.backward()
    assert torch.isfinite(loss) and st.grad.abs().max().item() > 0
    # the same encodings as a pre-encoded batch, same RNG state for noise / timesteps
    gen.manual_seed(11)
    pre = wf.encode_raw_batch(batch)
    assert tuple(pre["latents"].shape) == (2, 16, 2, 6, 8) and tuple(pre["prompt_embeds"].shape) == (2, cfg.max_text_seq_length, cfg.text_embed_dim)
    torch.manual_seed(5)
    loss2 = wf.training_step(pre)
    assert abs(loss2.item() - loss.item()) < 2e-2 * abs(loss.item()), (loss.item(), loss2.item())
    # and one batch ahead on the side stream
    gen.manual_seed(11)
    it = iter(EncoderPrefetcher([batch, batch], encode=wf.encode_raw_batch, device=dev))
    first = next(it)
    torch.manual_seed(5)
    loss3 = wf.training_step(first)
    assert abs(loss3.item() - loss.item()) < 2e-2 * abs(loss.item()), (loss.item(), loss3.item())
    assert len(list(it)) == 1
