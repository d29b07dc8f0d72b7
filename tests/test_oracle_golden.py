"""CPU: pin the oracle (oracle/cogvideox_oracle.py) to the golden vectors generated from the reference's own modules
(tests/golden/make_golden.py).  fp32/fp64 restatements -> tight tolerances."""
import os

import numpy as np
import torch
import torch.nn.functional as F

import cogvideox_oracle as O
import golden_io

G = os.path.join(os.path.dirname(__file__), "golden")


def _sinusoid_bound(t, dim, max_period=10000.0):
    """1e-6 plus what the fp32 frequency table admits: exp() in fp32 is faithful to 1-2 ulps, which ones depends on the CPU's vector-math
    path (the golden holds one machine's), and an ulp of f moves the argument t*f, hence its sine and cosine, by up to |t f| 2^-23.  Any
    formula error (period, shift, flip, order) is off by orders of magnitude more."""
    half = dim // 2
    f = np.exp(-np.log(max_period) * np.arange(half) / half)
    tf = np.abs(np.asarray(t, np.float64)[:, None] * f[None])
    return 1e-6 + 4.0 * 2.0 ** -24 * np.concatenate([tf, tf], axis=1)


def test_timestep_sinusoid_matches_reference():
    g = np.load(os.path.join(G, "timestep_embedding.npz"))
    t = torch.from_numpy(g["t"])
    for dim, key in ((1920, "emb1920"), (64, "emb64")):
        dev = np.abs(O.timestep_sinusoid(t, dim).numpy().astype(np.float64) - g[key])
        assert (dev <= _sinusoid_bound(g["t"], dim)).all(), (dim, dev.max())


def test_pos_embed_matches_sat_twin():
    g = np.load(os.path.join(G, "pos_embed_3d.npz"))
    assert np.abs(O.sincos_pos_embed_3d(128, 6, 8, 3, 1.875, 1.0) - g["small"]).max() < 1e-12
    full = O.sincos_pos_embed_3d(1920, 30, 45, 13, 1.875, 1.0).reshape(-1, 1920)
    assert np.abs(full[g["full_rows_idx"]] - g["full_rows"]).max() < 1e-12
    assert np.abs(full.sum(0) - g["full_colsum"]).max() < 1e-8 and np.abs(full.sum(1) - g["full_rowsum"]).max() < 1e-8
    # the table the product builds is the same function (host-side numpy, not a kernel)
    from vt355.dit import sincos_pos_embed_3d
    assert np.abs(sincos_pos_embed_3d(128, 6, 8, 3, 1.875, 1.0).reshape(3, 48, 128) - g["small"]).max() < 1e-12


def test_schedule_matches_zero_snr_discretizer():
    g = np.load(os.path.join(G, "schedule_cogvideox.npz"))
    for s in (1, 3):
        ab = O.alphas_cumprod_cogvideox(snr_shift_scale=float(s))
        assert np.abs(ab.sqrt().numpy() - g[f"sqrt_abar_shift{s}"]).max() < 2e-7      # reference rescales in fp32
    assert O.alphas_cumprod_cogvideox()[-1].item() == 0.0
    from vt355.scheduler import CogVideoXDPMScheduler
    assert torch.equal(CogVideoXDPMScheduler().alphas_cumprod, O.alphas_cumprod_cogvideox())


def test_qsample_getv_match_ddpm():
    g = np.load(os.path.join(G, "ddpm_qsample_getv.npz"))
    abar = torch.from_numpy(g["alphas_cumprod"]).float()
    x0, nz, t = torch.from_numpy(g["x0"]), torch.from_numpy(g["noise"]), torch.from_numpy(g["t"])
    assert (O.add_noise(x0, nz, t, abar) - torch.from_numpy(g["q_sample"])).abs().max() < 2e-6
    assert (O.get_velocity(x0, nz, t, abar) - torch.from_numpy(g["get_v"])).abs().max() < 2e-6


def test_modulate_and_unpatchify_conventions():
    g = np.load(os.path.join(G, "modulate_unpatchify.npz"))
    x, sh, sc = [torch.from_numpy(g[k]) for k in ("x", "shift", "scale")]
    assert torch.equal(x * (1 + sc[:, None]) + sh[:, None], torch.from_numpy(g["modulated"]))
    tok = torch.from_numpy(g["tokens"])
    out = tok.reshape(2, 3, 2, 4, -1, 2, 2).permute(0, 1, 4, 2, 5, 3, 6).flatten(5, 6).flatten(3, 4)   # oracle step 5
    assert torch.equal(out, torch.from_numpy(g["unpatchified"]))


def test_attention_with_qk_layernorm_matches_opensora_attention():
    g = np.load(os.path.join(G, "opensora_primitives.npz"))
    x = torch.from_numpy(g["attn_x"])
    qkv = F.linear(x, torch.from_numpy(g["attn_qkv.weight"]), torch.from_numpy(g["attn_qkv.bias"]))
    q, k, v = qkv.view(2, 24, 3, 2, 64).permute(2, 0, 3, 1, 4).unbind(0)
    q = F.layer_norm(q, (64,), torch.from_numpy(g["attn_q_norm.weight"]), torch.from_numpy(g["attn_q_norm.bias"]), 1e-5)
    k = F.layer_norm(k, (64,), torch.from_numpy(g["attn_k_norm.weight"]), torch.from_numpy(g["attn_k_norm.bias"]), 1e-5)
    o, _ = O.attention(q, k, v)
    y = F.linear(o.transpose(1, 2).reshape(2, 24, 128), torch.from_numpy(g["attn_proj.weight"]), torch.from_numpy(g["attn_proj.bias"]))
    assert (y - torch.from_numpy(g["attn_y"])).abs().max() < 1e-5
    # modulate and GELU-tanh MLP primitives
    xm = torch.from_numpy(g["mod_x"])
    ym = F.layer_norm(xm, (128,), None, None, 1e-6) * (1 + torch.from_numpy(g["mod_scale"])) + torch.from_numpy(g["mod_shift"])
    assert (ym - torch.from_numpy(g["mod_y"])).abs().max() < 1e-5
    h = O.gelu_tanh(F.linear(xm, torch.from_numpy(g["mlp_fc1_w"]), torch.from_numpy(g["mlp_fc1_b"])))
    assert (F.linear(h, torch.from_numpy(g["mlp_fc2_w"]), torch.from_numpy(g["mlp_fc2_b"])) - torch.from_numpy(g["mlp_y"])).abs().max() < 1e-5


def test_attention_matches_lvdm_crossattention():
    g = np.load(os.path.join(G, "lvdm_crossattention.npz"))
    x = torch.from_numpy(g["x"])
    q, k, v = [F.linear(x, torch.from_numpy(g[f"to_{n}_weight"])).view(2, 20, 2, 64).transpose(1, 2) for n in "qkv"]
    o, _ = O.attention(q, k, v)
    y = F.linear(o.transpose(1, 2).reshape(2, 20, 128), torch.from_numpy(g["to_out_0_weight"]), torch.from_numpy(g["to_out_0_bias"]))
    assert (y - torch.from_numpy(g["y"])).abs().max() < 1e-5


def test_oracle_train_step_runs_and_lora_zero_init_is_identity():
    cfg = O.tiny_config()
    P = O.init_params(cfg, 0)
    B, Fr = 2, (cfg.sample_frames - 1) // 4 + 1
    g = torch.Generator().manual_seed(0)
    x0 = torch.randn(B, Fr, 16, cfg.sample_height, cfg.sample_width, generator=g)
    txt = torch.randn(B, cfg.max_text_seq_length, cfg.text_embed_dim, generator=g)
    nz, t, abar = torch.randn(x0.shape, generator=g), torch.tensor([3, 900]), O.alphas_cumprod_cogvideox()
    l0 = O.training_loss(P, cfg, x0, txt, nz, t, abar.float())
    l1 = O.training_loss(P, cfg, x0, txt, nz, t, abar.float(), O.init_lora(cfg))        # B = 0 -> same loss
    assert torch.isfinite(l0) and torch.allclose(l0, l1)
    # AdamW restatement == torch.optim.AdamW
    p = torch.randn(100, generator=g); gr = torch.randn(100, generator=g)
    pt = p.clone().requires_grad_(True); opt = torch.optim.AdamW([pt], lr=1e-2)
    m, v = torch.zeros(100), torch.zeros(100)
    for i in range(3):
        pt.grad = gr.clone(); opt.step(); O.adamw_step(p, gr, m, v, i + 1, 1e-2)
    assert torch.allclose(p, pt.detach(), atol=1e-6)


def test_rope_tables_and_rotation_match_sat_mixin():
    """tests/golden/rope_3d.npz: Rotary3DPositionEmbeddingMixin tables + rotary() (dit_video_concat.py:263-341)."""
    g = np.load(os.path.join(G, "rope_3d.npz"))
    cos, sin = O.rope_3d_tables(64, ((0, 0), (4, 5)), (4, 5), 3)
    np.testing.assert_allclose(cos.numpy(), g["small_cos"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(sin.numpy(), g["small_sin"], rtol=0, atol=1e-6)
    rot = O.apply_rope(torch.from_numpy(g["x"]), cos, sin)
    np.testing.assert_allclose(rot.numpy(), g["rotated"], rtol=0, atol=1e-6)
    # full CogVideoX-5B grid 13 x 30 x 45 (49 x 480 x 720): the crop region is the whole base grid
    crop = O.resize_crop_region_for_grid((30, 45), (30, 45))
    assert crop == ((0, 0), (30, 45))
    cos, sin = O.rope_3d_tables(64, crop, (30, 45), 13)
    assert cos.shape == (17550, 64)
    idx = g["full_rows_idx"]
    # fp32 cos/sin of angles up to 44 rad: the two constructions may differ in the last ulp of the angle
    np.testing.assert_allclose(cos[idx].numpy(), g["full_cos_rows"], rtol=0, atol=5e-6)
    np.testing.assert_allclose(sin[idx].numpy(), g["full_sin_rows"], rtol=0, atol=5e-6)
    np.testing.assert_allclose(cos.double().sum(0).numpy(), g["full_cos_colsum"], rtol=0, atol=2e-2)
    np.testing.assert_allclose(sin.double().sum(0).numpy(), g["full_sin_colsum"], rtol=0, atol=2e-2)


def test_crop_region_matches_reference():
    g = np.load(os.path.join(G, "crop_region.npz"))
    for src, tgt, reg in zip(g["src"], g["tgt"], g["region"]):
        got = O.resize_crop_region_for_grid(tuple(int(v) for v in src), tuple(int(v) for v in tgt))
        assert np.array_equal(np.array(got), reg), (src, tgt, got, reg)


def test_rope_block_is_orthogonal_and_position_relative():
    """size-independent properties of the rotation: norm preserving; q.k depends only on the position difference
    along an axis (here: the frame axis, spatial position fixed)."""
    cos, sin = O.rope_3d_tables(64, ((0, 0), (2, 2)), (2, 2), 6)
    x = torch.randn(1, 1, 24, 64, dtype=torch.float64)
    r = O.apply_rope(x, cos.double(), sin.double())
    np.testing.assert_allclose(r.norm(dim=-1).numpy(), x.norm(dim=-1).numpy(), rtol=1e-6)   # fp32 tables: cos^2+sin^2 = 1 +- 1e-7
    q = torch.randn(64, dtype=torch.float64).expand(24, 64)
    k = torch.randn(64, dtype=torch.float64).expand(24, 64)
    rq, rk = O.apply_rope(q, cos.double(), sin.double()), O.apply_rope(k, cos.double(), sin.double())
    # tokens (t, 0, 0) are rows 4t: <R_t q, R_{t+2} k> must not depend on t
    dots = [float(rq[4 * t] @ rk[4 * (t + 2)]) for t in range(4)]
    assert max(dots) - min(dots) < 1e-5


def test_t5_oracle_matches_transformers_golden():
    """oracle/t5_oracle.py against the output of transformers' own T5EncoderModel on seeded weights
    (tests/golden/make_golden_t5.py): the whole encoder and the bucketed relative position bias (150 tokens > max_distance,
    so exact, log-spaced and clamped buckets all occur)."""
    import t5_oracle as T
    g = golden_io.load("t5_tiny")
    cfg = T.tiny_config()
    P = {k[2:]: torch.from_numpy(g[k]).double() for k in g.files if k.startswith("P.")}
    ids = torch.from_numpy(g["ids"])
    out = T.encoder_forward(P, cfg, ids)
    ref = torch.from_numpy(g["out"]).double()
    assert (out - ref).abs().max().item() < 2e-5 * ref.abs().max().item()
    bias = T.position_bias(P["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], ids.shape[1], cfg)
    assert torch.equal(bias.float(), torch.from_numpy(g["bias"]))
    # bucketing known answers: 0 -> 0, +1 -> 17, -1 -> 1, far left / right clamp to 15 / 31
    rel = torch.tensor([0, 1, -1, 7, -8, 200, -200])
    assert T.relative_position_bucket(rel, 32, 128).tolist() == [0, 17, 1, 23, 8, 31, 15]


def test_vae_encoder_oracle_matches_reference_twin_golden():
    """oracle/vae_oracle.py against the output of the reference's own ContextParallelEncoder3D (cogvideo_sat/vae_modules/
    cp_enc_dec.py:779-907) on seeded weights (tests/golden/make_golden_vae.py): causal padding, ResNet blocks, temporal + spatial
    downsampling, 9 frames -> 3 latent frames."""
    import vae_oracle as V
    g = golden_io.load("vae_encoder_tiny")
    cfg = V.tiny_config()
    P = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("P.")}
    out = V.encoder_forward(P, cfg, torch.from_numpy(g["x"]))
    ref = torch.from_numpy(g["out"])
    assert out.shape == ref.shape == (1, 8, 3, 4, 6)
    assert (out - ref).abs().max().item() < 1e-5 * ref.abs().max().item()
    mom = torch.randn(2, 8, 3, 4, 6)
    eps = torch.randn(2, 4, 3, 4, 6)
    lat = V.sample_latent(mom, eps, 0.7)
    assert torch.allclose(lat, (mom[:, :4] + torch.exp(0.5 * mom[:, 4:].clamp(-30, 20)) * eps) * 0.7)


def test_vae_downsample_both_temporal_branches_match_reference_twin():
    """DownSample3D (cp_enc_dec.py:640-676) run alone by tests/golden/make_golden_vae.py: the rank-0 / fake_cp branch (first frame
    kept, pairs after it) and the plain avg_pool1d branch, odd and even frame counts.  The encoder follows diffusers' rule: odd ->
    keep first, even -> plain pairs (even frame counts used to take the odd rule silently)."""
    import vae_oracle as V
    g = np.load(os.path.join(G, "vae_downsample3d.npz"))
    P = {"d.conv.weight": torch.from_numpy(g["ds.conv.weight"]), "d.conv.bias": torch.from_numpy(g["ds.conv.bias"])}
    for T in (9, 8, 4):
        x = torch.from_numpy(g[f"x{T}"])
        kf = V.downsample(x, P, "d.", True, keep_first=True)
        ap = V.downsample(x, P, "d.", True, keep_first=False)
        assert torch.equal(kf, torch.from_numpy(g[f"keep_first{T}"])), T
        assert torch.equal(ap, torch.from_numpy(g[f"all_pairs{T}"])), T
        auto = V.downsample(x, P, "d.", True)
        assert torch.equal(auto, kf if T % 2 else ap)


def test_dit_block_and_final_layer_composition_match_sat_twin():
    """The oracle's CogVideoXBlock / final-layer WIRING against the reference's in-tree SAT twin run by
    tests/golden/make_golden_dit_block.py: AdaLNMixin.layer_forward + attention_fn (dit_video_concat.py:577-701) and
    FinalLayerMixin.final_forward (:478-498).  The twin's 12-way adaLN chunk (shift,scale,gate)x{msa,mlp} for video then text
    is mapped onto diffusers' two 6-way CogVideoXLayerNormZero linears (norm1: msa, norm2: mlp; video chunks first)."""
    g = np.load(os.path.join(G, "sat_dit_block.npz"))
    T = lambda k: torch.from_numpy(g[k]).double()
    St, heads = int(g["St"]), int(g["heads"])
    d = g["hidden"].shape[2]
    te = g["emb"].shape[1]
    cfg = O.DiTConfig(num_layers=1, num_attention_heads=heads, attention_head_dim=d // heads, time_embed_dim=te, out_channels=4,
                      in_channels=4)
    assert cfg.norm_eps == 1e-5 and cfg.qk_norm_eps == 1e-6
    W, Bv = T("w.adaLN_modulations.0.1.weight").view(12, d, te), T("w.adaLN_modulations.0.1.bias").view(12, d)
    pre = "transformer_blocks.0."
    P = {}
    for name, idx in (("norm1", [0, 1, 2, 6, 7, 8]), ("norm2", [3, 4, 5, 9, 10, 11])):
        P[pre + name + ".linear.weight"] = W[idx].reshape(6 * d, te)
        P[pre + name + ".linear.bias"] = Bv[idx].reshape(6 * d)
    P[pre + "norm1.norm.weight"], P[pre + "norm1.norm.bias"] = T("w.layer.input_layernorm.weight"), T("w.layer.input_layernorm.bias")
    P[pre + "norm2.norm.weight"], P[pre + "norm2.norm.bias"] = T("w.layer.post_attention_layernorm.weight"), T("w.layer.post_attention_layernorm.bias")
    qkv_w, qkv_b = T("w.layer.attention.query_key_value.weight"), T("w.layer.attention.query_key_value.bias")
    for i, n in enumerate(("to_q", "to_k", "to_v")):
        P[pre + f"attn1.{n}.weight"], P[pre + f"attn1.{n}.bias"] = qkv_w[i * d:(i + 1) * d], qkv_b[i * d:(i + 1) * d]
    P[pre + "attn1.to_out.0.weight"], P[pre + "attn1.to_out.0.bias"] = T("w.layer.attention.dense.weight"), T("w.layer.attention.dense.bias")
    P[pre + "attn1.norm_q.weight"], P[pre + "attn1.norm_q.bias"] = T("w.query_layernorm_list.0.weight"), T("w.query_layernorm_list.0.bias")
    P[pre + "attn1.norm_k.weight"], P[pre + "attn1.norm_k.bias"] = T("w.key_layernorm_list.0.weight"), T("w.key_layernorm_list.0.bias")
    P[pre + "ff.net.0.proj.weight"], P[pre + "ff.net.0.proj.bias"] = T("w.layer.mlp.dense_h_to_4h.weight"), T("w.layer.mlp.dense_h_to_4h.bias")
    P[pre + "ff.net.2.weight"], P[pre + "ff.net.2.bias"] = T("w.layer.mlp.dense_4h_to_h.weight"), T("w.layer.mlp.dense_4h_to_h.bias")
    hid, emb = T("hidden"), T("emb")
    # the twin feeds emb through its own nn.SiLU inside adaLN_modulations; so does the oracle's ln_zero
    ht, hv = O.dit_block(hid[:, :St], hid[:, St:], emb, P, pre, cfg)
    out = torch.cat([ht, hv], dim=1)
    ref = T("out")
    assert (out - ref).abs().max().item() < 1e-5 * ref.abs().max().item(), (out - ref).abs().max().item()
    # ---- final layer: the twin has ONE LayerNorm (eps 1e-6) where diffusers has norm_final + norm_out.norm; with an identity
    # affine on norm_final the second LayerNorm of an already normalised row is the identity to O(eps)
    import dataclasses
    cfgf = dataclasses.replace(cfg, norm_eps=1e-6)
    Pf = {"norm_final.weight": torch.ones(d, dtype=torch.float64), "norm_final.bias": torch.zeros(d, dtype=torch.float64),
          "norm_out.norm.weight": T("f.norm_final.weight"), "norm_out.norm.bias": T("f.norm_final.bias"),
          "norm_out.linear.weight": T("f.adaLN_modulation.1.weight"), "norm_out.linear.bias": T("f.adaLN_modulation.1.bias"),
          "proj_out.weight": T("f.linear.weight"), "proj_out.bias": T("f.linear.bias")}
    Tn, Hp, Wp = [int(v) for v in g["grid"]]
    img = O.dit_final(ref[:, St:], emb, Pf, cfgf, Tn, 2 * Hp, 2 * Wp)
    fref = T("final_out")
    assert img.shape == fref.shape
    assert (img - fref).abs().max().item() < 1e-5 * fref.abs().max().item(), (img - fref).abs().max().item()


# ------------------------------------------------------------------------------------------------ VideoCrafter2 UNet
def _unet_params():
    import unet_oracle as U
    cfg = U.tiny_config()
    return U, cfg, {k: v.double() for k, v in U.init_params(cfg, seed=11).items()}


def _sub(P, pre):
    return {k: v for k, v in P.items() if k.startswith(pre)}


def test_unet_oracle_matches_reference_unet_output_and_gradients():
    """oracle/unet_oracle.py vs the reference's own UNetModel (openaimodel3d.py:313-694) run by tests/golden/make_golden_unet.py:
    output, eps-MSE loss, checksums of ALL 626 parameter gradients and 15 gradients in full."""
    U, cfg, P = _unet_params()
    g = golden_io.load("unet_tiny")
    for v in P.values():
        v.requires_grad_(True)
    T = lambda k: torch.from_numpy(g[k])
    out = U.unet_forward(P, cfg, T("x").double(), T("t"), T("context").double(), fps=T("fps"))
    ref = T("out").double()
    assert (out - ref).abs().max().item() < 2e-5 * ref.abs().max().item()
    loss = U.lvdm_loss(out, T("noise").double())
    assert abs(loss.item() - float(g["loss"])) < 1e-5 * float(g["loss"])
    loss.backward()
    names = list(P)
    gs = np.array([P[n].grad.sum().item() for n in names]); ga = np.array([P[n].grad.abs().sum().item() for n in names])
    assert np.allclose(ga, g["grad_abs_sum"], rtol=2e-4, atol=1e-7), np.abs(ga - g["grad_abs_sum"]).max()
    assert np.allclose(gs, g["grad_sum"], rtol=0, atol=2e-4 * np.abs(g["grad_abs_sum"]).max())
    full = [k[5:] for k in g.files if k.startswith("grad.")]
    assert len(full) == 15
    for n in full:
        r = torch.from_numpy(g["grad." + n]).double()
        assert (P[n].grad - r).abs().max().item() < 2e-4 * r.abs().max().item() + 1e-9, n


def test_unet_oracle_blocks_match_reference_blocks():
    """each block alone (ResBlock with temporal conv + 1x1 skip, TemporalConvBlock, SpatialTransformer, TemporalTransformer,
    CrossAttention with a context longer than 77, Downsample, Upsample): output, input gradients, every parameter gradient"""
    U, cfg, P = _unet_params()
    g = golden_io.load("unet_blocks")
    T = lambda k: torch.from_numpy(g[k]).double()

    def check(tag, pre, fn, nin):
        for v in P.values():
            v.grad = None
            v.requires_grad_(True)
        ins = [T(f"{tag}.in{i}").requires_grad_(True) for i in range(nin)]
        y = fn(*ins)
        ref = T(tag + ".y")
        assert (y - ref).abs().max().item() < 2e-5 * ref.abs().max().item(), tag
        (y * T(tag + ".gy")).sum().backward()
        for i in range(nin):
            r = T(f"{tag}.gin{i}")
            assert (ins[i].grad - r).abs().max().item() < 1e-4 * r.abs().max().item(), (tag, i)
        keys = [k for k in g.files if k.startswith(tag + ".g.")]
        assert keys
        for k in keys:
            r = T(k)
            got = P[pre + k[len(tag) + 3:]].grad
            assert (got - r).abs().max().item() < 1e-4 * r.abs().max().item() + 1e-10, k

    check("res", "input_blocks.3.0.", lambda a, e: U.res_block(a, e, P, "input_blocks.3.0", 2, True), 2)
    check("tconv", "input_blocks.1.0.temopral_conv.", lambda a: U.temporal_conv_block(a, P, "input_blocks.1.0.temopral_conv"), 1)
    check("st", "input_blocks.1.1.", lambda a, c: U.spatial_transformer(a, c, P, "input_blocks.1.1", 1), 2)
    check("tt", "input_blocks.1.2.", lambda a: U.temporal_transformer(a, P, "input_blocks.1.2", 1), 1)
    check("xattn", "input_blocks.1.1.transformer_blocks.0.attn2.",
          lambda a, c: U.cross_attention(a, P, "input_blocks.1.1.transformer_blocks.0.attn2", 1, c), 2)
    check("down", "input_blocks.2.0.", lambda a: U._run_block([("down", "input_blocks.2.0", {})], a, None, None, 1, P, cfg), 1)
    check("up", "output_blocks.1.3.", lambda a: U._run_block([("up", "output_blocks.1.3", {})], a, None, None, 1, P, cfg), 1)


def test_philox_known_answer_vectors_and_keep_rate():
    """oracle/philox.py against Random123's philox4x32-10 known-answer vectors (kat_vectors), and the keep mask's rate"""
    import philox
    kat = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for ctr, key, want in kat:
        assert [int(v) for v in philox.philox4x32_10(ctr, key)] == want
    m = philox.dropout_keep_mask(256, 320, 0.1, seed=77, offset=5 << 36)
    assert abs(m.mean() - 0.9) < 5e-3
    assert not np.array_equal(m, philox.dropout_keep_mask(256, 320, 0.1, seed=78, offset=5 << 36))
    assert np.array_equal(philox.dropout_keep_mask(4, 8, 0.0, 1), np.ones((4, 8), np.uint8))


def test_unet_oracle_train_mode_dropout_matches_reference():
    """TemporalConvBlock and the whole UNetModel of the reference under .train() with their REAL nn.Dropout(0.1) modules
    (tests/golden/make_golden_unet_train.py recorded the keep masks they drew): the oracle with those masks reproduces output, input
    gradient and parameter gradients -- pins WHERE the dropout sits (GroupNorm -> SiLU -> Dropout -> Conv3d, conv2..conv4) and its 1 / (1 - p)"""
    U, cfg, P = _unet_params()
    g = golden_io.load("unet_train")
    T = lambda k: torch.from_numpy(g[k]).double()
    pre = "input_blocks.1.0.temopral_conv"
    masks = {k[len("tconv.mask."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("tconv.mask.")}
    assert set(masks) == {f"{pre}.conv{j}" for j in (2, 3, 4)}
    for v in P.values():
        v.grad = None; v.requires_grad_(True)
    x = T("tconv.x").requires_grad_(True)
    y = U.temporal_conv_block(x, P, pre, masks)
    assert (y - T("tconv.y")).abs().max().item() < 2e-5 * T("tconv.y").abs().max().item()
    (y * T("tconv.gy")).sum().backward()
    assert (x.grad - T("tconv.gx")).abs().max().item() < 1e-4 * T("tconv.gx").abs().max().item()
    for k in [k for k in g.files if k.startswith("tconv.g.")]:
        r = T(k)
        assert (P[pre + "." + k[len("tconv.g."):]].grad - r).abs().max().item() < 1e-4 * r.abs().max().item() + 1e-10, k
    eval_y = U.temporal_conv_block(T("tconv.x"), P, pre, None)
    assert (eval_y - T("tconv.y")).abs().max().item() > 1e-3                     # the masks matter
    # ---- whole network ----
    for v in P.values():
        v.grad = None
    nm = {}
    for k in g.files:
        if k.startswith("net.mask."):
            shp = tuple(int(v) for v in g["net.maskshape." + k[len("net.mask."):]])
            nm[k[len("net.mask."):]] = torch.from_numpy(np.unpackbits(g[k])[:int(np.prod(shp))].reshape(shp))
    assert len(nm) == 24
    out = U.unet_forward(P, cfg, T("net.x"), torch.from_numpy(g["net.t"]), T("net.context"), fps=torch.from_numpy(g["net.fps"]), dropout_masks=nm)
    assert (out - T("net.out")).abs().max().item() < 5e-5 * T("net.out").abs().max().item()
    loss = U.lvdm_loss(out, T("net.noise"))
    assert abs(loss.item() - float(g["net.loss"])) < 1e-5 * float(g["net.loss"])
    loss.backward()
    gs = np.array([float(v.grad.sum()) for v in P.values()]); ga = np.array([float(v.grad.abs().sum()) for v in P.values()])
    assert np.allclose(ga, g["net.grad_abs_sum"], rtol=2e-4, atol=1e-9)
    assert np.allclose(gs, g["net.grad_sum"], rtol=2e-3, atol=2e-4 * np.abs(g["net.grad_abs_sum"]).max())


def test_unet_oracle_lora_matches_reference_with_hand_injected_adapters():
    """peft is absent offline: tests/golden/make_golden_unet_train.py wrapped to_q / to_k / to_v of every CrossAttention of the REFERENCE
    UNetModel with peft's Linear formula y = W x + (lora_alpha / r) B(A x) (vc2_t2v_lora.yaml:7-12; ddpm3d.py:100-117, 434-445), base
    frozen.  The oracle with the same adapters: output, loss, all 180 adapter gradients."""
    U, cfg, P = _unet_params()
    g = golden_io.load("unet_train")
    T = lambda k: torch.from_numpy(g[k]).double()
    L = U.init_lora(cfg, r=int(g["lora.r"]), lora_alpha=float(g["lora.alpha"]), seed=3, zero_b=False)
    assert len(U.lora_sites(cfg)) == 90
    Lp = {k: (v.double().requires_grad_(True) if torch.is_tensor(v) else v) for k, v in L.items()}
    out = U.unet_forward({**P, **Lp}, cfg, T("net.x"), torch.from_numpy(g["net.t"]), T("net.context"), fps=torch.from_numpy(g["net.fps"]))
    assert (out - T("lora.out")).abs().max().item() < 5e-5 * T("lora.out").abs().max().item()
    loss = U.lvdm_loss(out, T("net.noise"))
    assert abs(loss.item() - float(g["lora.loss"])) < 1e-5 * float(g["lora.loss"])
    loss.backward()
    keys = [k for k in g.files if k.startswith("lora.g.")]
    assert len(keys) == 180
    for k in keys:
        r = T(k)
        got = Lp[k[len("lora.g."):]].grad
        assert (got - r).abs().max().item() < 2e-4 * r.abs().max().item() + 1e-12, k


def test_lvdm_schedule_and_q_sample_match_reference():
    import unet_oracle as U
    g = np.load(os.path.join(G, "unet_loss.npz"))
    ab = U.lddpm_alphas_cumprod()
    assert np.allclose(ab.numpy(), g["alphas_cumprod"], rtol=1e-6)
    xn = U.q_sample(torch.from_numpy(g["x0"]), torch.from_numpy(g["t"]), torch.from_numpy(g["noise"]), ab)
    assert np.allclose(xn.numpy(), g["q_sample"], rtol=1e-5, atol=1e-6)
    sa = U.scale_arr()
    assert sa.shape[0] == 1400 and abs(sa[0].item() - 1.0) < 1e-7 and abs(sa[399].item() - 0.7) < 1e-7 and abs(sa[999].item() - 0.7) < 1e-7


# ------------------------------------------------------------------------------------------------ OpenSora STDiT
def test_stdit_oracle_matches_reference_stdit():
    """oracle/stdit_oracle.py vs the reference's own STDiT (stdit.py:136-416) run by tests/golden/make_golden_stdit.py: output,
    checksums of all 53 parameter gradients, 10 gradients (rows), and the XL/2 positional tables at 16x256x256"""
    import stdit_oracle as SO
    cfg = SO.tiny_config()
    g = np.load(os.path.join(G, "stdit_tiny.npz"))
    P = {k: v.double().requires_grad_(True) for k, v in SO.init_params(cfg, seed=3).items()}
    T = lambda k: torch.from_numpy(g[k])
    assert np.allclose(SO.spatial_pos_embed(cfg).numpy(), g["pos_embed"][0], atol=1e-6)
    assert np.allclose(SO.temporal_pos_embed(cfg).numpy(), g["pos_embed_temporal"][0], atol=1e-6)
    out = SO.stdit_forward(P, cfg, T("x").double(), T("t"), T("y").double(), T("mask"))
    ref = T("out").double()
    assert out.dtype == torch.float32 and (out.double() - ref).abs().max().item() < 2e-5 * ref.abs().max().item()
    (out.double() * T("gy").double()).sum().backward()
    names = list(P)
    ga = np.array([P[n].grad.abs().sum().item() for n in names])
    assert np.allclose(ga, g["grad_abs_sum"], rtol=3e-4, atol=1e-6), np.abs(ga / g["grad_abs_sum"] - 1).max()
    for k in [k for k in g.files if k.startswith("grad.")]:
        r = torch.from_numpy(g[k]).double()
        got = P[k[5:]].grad.reshape(P[k[5:]].shape[0], -1)[:r.shape[0]]
        assert (got - r).abs().max().item() < 3e-4 * r.abs().max().item() + 1e-9, k
    xl = SO.STDiTConfig()
    pe, pt = SO.spatial_pos_embed(xl).double().numpy(), SO.temporal_pos_embed(xl).double().numpy()
    assert np.allclose(pe[[0, 1, 17, 255]], g["xl_pos_rows"], atol=1e-6) and np.allclose(pe.sum(0), g["xl_pos_colsum"], atol=1e-4)
    assert np.allclose(pt[[0, 1, 15]], g["xl_tpe_rows"], atol=1e-6) and np.allclose(pt.sum(0), g["xl_tpe_colsum"], atol=1e-4)


def test_opensora_loss_with_vb_term_matches_reference():
    """LatentDiffusion.p_losses + _vb_terms_bpd + OpenSoraScheduler.p_mean_variance (iddpm3d.py:1332-1413, 1543-1583, 444-519 incl. the
    inverted mean-type branch :497-500) executed from the reference file by the golden script: loss, its mse / vb parts, d loss / d model
    output (t = 0 decoder-NLL branch included), schedule tables"""
    import stdit_oracle as SO
    g = np.load(os.path.join(G, "stdit_loss.npz"))
    sch = SO.schedule(1000)
    assert np.array_equal(sch["betas"].numpy(), g["betas"]) and np.allclose(sch["alphas_cumprod"].numpy(), g["alphas_cumprod"], rtol=1e-6)
    assert np.allclose(sch["posterior_log_variance_clipped"].numpy(), g["posterior_log_variance_clipped"], rtol=1e-5)
    T = lambda k: torch.from_numpy(g[k])
    assert np.allclose(SO.q_sample(T("x0"), T("t"), T("noise"), sch).numpy(), g["x_t"], rtol=1e-5, atol=1e-6)
    mo = T("model_out").clone().requires_grad_(True)
    loss, mse, vb = SO.opensora_loss(mo, T("x0"), T("noise"), T("t"), sch)
    assert abs(loss.item() - float(g["loss"])) < 1e-5 * float(g["loss"])
    assert abs(mse.item() - float(g["loss_mse"])) < 1e-5 * float(g["loss_mse"]) and abs(vb.item() - float(g["loss_vb"])) < 1e-5 * float(g["loss_vb"])
    loss.backward()
    r = T("dmodel_out")
    assert (mo.grad - r).abs().max().item() < 1e-4 * r.abs().max().item()


# ------------------------------------------------------------------------------------------------ HunyuanVideo blocks
def test_hunyuan_block_oracle_matches_reference_blocks():
    """oracle/hunyuan_oracle.py vs the reference's own MMDoubleStreamBlock / MMSingleStreamBlock (hyvideo_t2v/modules/models.py:21-393) run by
    tests/golden/make_golden_hunyuan.py: outputs, input gradients (img, txt, vec), every parameter gradient (rows + checksums)"""
    import hunyuan_oracle as HO
    g = np.load(os.path.join(G, "hunyuan_blocks.npz"))
    T = lambda k: torch.from_numpy(g[k]).double()
    D, H = 256, 2
    cos, sin, tv = T("cos"), T("sin"), torch.from_numpy(g["txt_valid"])

    def check_grads(P, tag):
        for n, p in P.items():
            r = T(f"{tag}_g.{n}")
            got = p.grad.reshape(p.shape[0], -1)[:r.shape[0]]
            assert (got - r).abs().max().item() < 2e-4 * r.abs().max().item() + 1e-9, (tag, n)
            cs = g[f"{tag}_c.{n}"]
            assert abs(p.grad.abs().sum().item() - cs[1]) < 3e-4 * cs[1] + 1e-9, (tag, n)

    Pd = {k: v.double().requires_grad_(True) for k, v in HO.init(HO.double_block_shapes(D, H), 1).items()}
    img, txt, vec = T("img").requires_grad_(True), T("txt").requires_grad_(True), T("vec").requires_grad_(True)
    io, to = HO.double_block(img, txt, vec, Pd, "", H, tv, cos, sin)
    assert (io - T("d_img")).abs().max().item() < 2e-5 * T("d_img").abs().max().item()
    valid = (T("d_gt").abs().sum(-1, keepdim=True) > 0).double()
    assert ((to - T("d_txt")) * valid).abs().max().item() < 2e-5 * T("d_txt").abs().max().item()
    ((io * T("d_gi")).sum() + (to * T("d_gt")).sum()).backward()
    for got, k in ((img.grad, "d_dimg"), (txt.grad, "d_dtxt"), (vec.grad, "d_dvec")):
        assert (got - T(k)).abs().max().item() < 2e-4 * T(k).abs().max().item(), k
    check_grads(Pd, "d")

    Ps = {k: v.double().requires_grad_(True) for k, v in HO.init(HO.single_block_shapes(D, H), 2).items()}
    x = torch.cat([T("img"), T("txt")], 1).requires_grad_(True)
    v2 = T("vec").requires_grad_(True)
    xo = HO.single_block(x, v2, Ps, "", H, g["txt"].shape[1], tv, cos, sin)
    vm = (T("s_gx").abs().sum(-1, keepdim=True) > 0).double()
    assert ((xo - T("s_x")) * vm).abs().max().item() < 2e-5 * T("s_x").abs().max().item()
    (xo * T("s_gx")).sum().backward()
    assert (x.grad - T("s_dx")).abs().max().item() < 2e-4 * T("s_dx").abs().max().item()
    assert (v2.grad - T("s_dvec")).abs().max().item() < 2e-4 * T("s_dvec").abs().max().item()
    check_grads(Ps, "s")


def test_hunyuan_model_oracle_matches_reference_transformer():
    """oracle/hunyuan_oracle.py::transformer_forward / token_refiner vs the reference's own HYVideoDiffusionTransformer (embedders, token refiner
    with its mask, one double + one single block, final layer, unpatchify) imported at a tiny size by tests/golden/make_golden_hunyuan.py"""
    import hunyuan_oracle as HO
    g = np.load(os.path.join(G, "hunyuan_model.npz"))
    T = lambda k: torch.from_numpy(g[k])
    D, H = 256, 2
    P = {k: v.double() for k, v in HO.init_model(HO.model_shapes(D, H, 1, 1, 4, 4, (1, 2, 2), 64, 32), 3).items()}
    txt = HO.token_refiner(T("text_states").double(), T("t"), T("text_mask"), P, H)
    valid = T("text_mask").bool()
    assert (txt - T("txt_refined").double())[valid].abs().max().item() < 1e-5 * T("txt_refined").abs().max().item()
    out = HO.transformer_forward(P, T("x").double(), T("t"), T("text_states").double(), T("text_mask"), T("text_states_2").double(),
                                 T("cos").double(), T("sin").double(), H, 1, 1, (1, 2, 2), 4)
    assert tuple(out.shape) == tuple(g["out"].shape)
    assert (out - T("out").double()).abs().max().item() < 2e-5 * T("out").abs().max().item()
