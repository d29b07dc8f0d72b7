"""CPU restatements for the DynamiCrafter path (float64 / float32 PyTorch, no device code).

dual_attention_ref: the dual-context cross-attention of lvdm/modules/attention.py:45-170 (CrossAttention with img_cross_attention,
einsum path) with a hand-written backward, so that the tests can also build the WRONG variants a kernel is most likely to compute
(one joint softmax, frame 0's image keys everywhere, delta = dO.O for both segments) and prove the comparison tells them apart.

The DynamiCrafter UNet below reuses oracle/unet_oracle.py (the VideoCrafter2 restatement) for everything the two networks share.
"""
import math

import torch
import torch.nn.functional as F

import unet_oracle as U


def _heads(t, H):
    """[N, S, H*64] -> [N, H, S, 64]"""
    return t.view(t.shape[0], t.shape[1], H, 64).permute(0, 2, 1, 3)


def _merge(t):
    """[N, H, S, 64] -> [N, S, H*64]"""
    return t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], t.shape[1] * 64)


def dual_attention_ref(q, k, v, k_ip, v_ip, H, rows_per_frame, img_scale=1.0, scale=0.125, do=None, variant="exact"):
    """q [B, Sq, H*64]; text k, v [B, Sa, H*64]; image k_ip, v_ip [B * Sq / rows_per_frame, Sb, H*64]; do like q or None.

    Returns dict(o=..., and with do: dq, dk, dv, dk_ip, dv_ip) in float64, layouts like the inputs.
    variant: "exact" | "joint_softmax" (one softmax over Sa + Sb keys) | "frame0_image" (every frame meets the image keys of its
    sample's frame 0) | "delta_from_o" (the softmax-backward constant of BOTH segments taken as rowsum(dO * O))."""
    dt = torch.float64
    B, Sq, D = q.shape
    nf = Sq // rows_per_frame
    assert Sq == nf * rows_per_frame and k_ip.shape[0] == B * nf and D == H * 64
    Sa, Sb = k.shape[1], k_ip.shape[1]
    if variant == "frame0_image":
        idx = (torch.arange(B * nf) // nf) * nf
        k_ip, v_ip = k_ip[idx], v_ip[idx]
    # one "item" per (sample, frame): queries [N, H, rpf, 64], text keys repeated over frames, that frame's image keys
    qh = _heads(q.to(dt).reshape(B * nf, rows_per_frame, D), H)
    ka = _heads(k.to(dt), H).repeat_interleave(nf, dim=0)
    va = _heads(v.to(dt), H).repeat_interleave(nf, dim=0)
    kb, vb = _heads(k_ip.to(dt), H), _heads(v_ip.to(dt), H)
    sa = torch.einsum("nhid,nhjd->nhij", qh, ka) * scale
    sb = torch.einsum("nhid,nhjd->nhij", qh, kb) * scale
    if variant == "joint_softmax":
        pj = torch.cat([sa, sb], dim=-1).softmax(-1)
        pa, pb = pj[..., :Sa], pj[..., Sa:]
    else:
        pa, pb = sa.softmax(-1), sb.softmax(-1)
    o = torch.einsum("nhij,nhjd->nhid", pa, va) + img_scale * torch.einsum("nhij,nhjd->nhid", pb, vb)
    out = {"o": _merge(o).reshape(B, Sq, D)}
    if do is None:
        return out
    g = _heads(do.to(dt).reshape(B * nf, rows_per_frame, D), H)
    dpa = torch.einsum("nhid,nhjd->nhij", g, va)
    dpb = img_scale * torch.einsum("nhid,nhjd->nhij", g, vb)
    if variant == "delta_from_o":
        da = db = (g * o).sum(-1, keepdim=True)
    else:
        da, db = (pa * dpa).sum(-1, keepdim=True), (pb * dpb).sum(-1, keepdim=True)
    dsa, dsb = pa * (dpa - da) * scale, pb * (dpb - db) * scale
    dq = torch.einsum("nhij,nhjd->nhid", dsa, ka) + torch.einsum("nhij,nhjd->nhid", dsb, kb)
    dka = torch.einsum("nhij,nhid->nhjd", dsa, qh)
    dva = torch.einsum("nhij,nhid->nhjd", pa, g)
    out["dq"] = _merge(dq).reshape(B, Sq, D)
    out["dk"] = _merge(dka).reshape(B, nf, Sa, D).sum(1)          # the text keys are shared by the sample's frames
    out["dv"] = _merge(dva).reshape(B, nf, Sa, D).sum(1)
    out["dk_ip"] = _merge(torch.einsum("nhij,nhid->nhjd", dsb, qh))
    out["dv_ip"] = _merge(img_scale * torch.einsum("nhij,nhid->nhjd", pb, g))
    return out


def dual_attention_autograd(q, k, v, k_ip, v_ip, H, rows_per_frame, img_scale, do, scale=0.125):
    """The same function as the reference module writes it (two softmaxes, summed), differentiated by autograd: float64."""
    dt = torch.float64
    B, Sq, D = q.shape
    nf = Sq // rows_per_frame
    leaves = [t.to(dt).clone().requires_grad_(True) for t in (q, k, v, k_ip, v_ip)]
    qq, kk, vv, ki, vi = leaves
    qh = _heads(qq.reshape(B * nf, rows_per_frame, D), H)
    ka, va = _heads(kk, H).repeat_interleave(nf, dim=0), _heads(vv, H).repeat_interleave(nf, dim=0)
    sim = torch.einsum("nhid,nhjd->nhij", qh, ka) * scale
    o = torch.einsum("nhij,nhjd->nhid", sim.softmax(-1), va)
    sim_ip = torch.einsum("nhid,nhjd->nhij", qh, _heads(ki, H)) * scale
    o = o + img_scale * torch.einsum("nhij,nhjd->nhid", sim_ip.softmax(-1), _heads(vi, H))
    o = _merge(o).reshape(B, Sq, D)
    (o * do.to(dt)).sum().backward()
    return {"o": o.detach(), "dq": qq.grad, "dk": kk.grad, "dv": vv.grad, "dk_ip": ki.grad, "dv_ip": vi.grad}


# ---------------------------------------------------------------------------------------------------------------------
# DynamiCrafter UNet (openaimodel3d_dc.py): oracle/unet_oracle.py's VideoCrafter2 restatement with the four additions --
# image branch in every spatial attn2, per-frame image context, fs conditioning through fps_embedding, 8 input channels
# ---------------------------------------------------------------------------------------------------------------------
IMG_TOKENS = 16          # image tokens per frame (Resampler num_queries), the reference's hard-coded 77 + t * 16 split


def dc_tiny_config(**kw):
    """tiny_config of the VideoCrafter2 oracle with 8 input channels; fps_cond=True carries the fps_embedding that fs_condition feeds"""
    base = dict(in_channels=8, fps_cond=True)
    base.update(kw)
    return U.tiny_config(**base)


def _spatial_prefixes(cfg):
    st = U.structure(cfg)
    layers = [l for blk in st["input"] for l in blk] + list(st["middle"]) + [l for blk in st["output"] for l in blk]
    return [pre for kind, pre, _ in layers if kind == "st"]


def dc_param_shapes(cfg):
    """state_dict keys of openaimodel3d_dc.UNetModel(img_cross_attention=True, fs_condition=True) in registration order: the
    VideoCrafter2 list with to_k_ip / to_v_ip after to_out of every SPATIAL attn2"""
    spatial = set(_spatial_prefixes(cfg))
    out = {}
    for k, s in U.param_shapes(cfg).items():
        out[k] = s
        if k.endswith(".attn2.to_out.0.bias") and k.split(".transformer_blocks.")[0] in spatial:
            pre = k[:-len("to_out.0.bias")]
            out[pre + "to_k_ip.weight"] = out[pre + "to_k.weight"]
            out[pre + "to_v_ip.weight"] = out[pre + "to_v.weight"]
    return out


def dc_init_params(cfg, seed=0, dtype=torch.float32):
    """seeded init as unet_oracle.init_params (nothing left at the reference's zero init: fps_embedding[-1], proj_out, ...)"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, s in dc_param_shapes(cfg).items():
        if len(s) == 1:
            w = torch.randn(s, generator=g) * 0.1 + (1.0 if k.endswith("weight") else 0.0)
        else:
            w = torch.randn(s, generator=g) * (0.7 / math.sqrt(math.prod(s[1:])))
        out[k] = w.to(dtype)
    return out


def dc_cross_attention(x, P, pre, heads, context, text_len=77, img_scale=1.0):
    """CrossAttention.forward with img_cross_attention, einsum path (attention.py:101-170): context = text rows then image rows"""
    lin = lambda t, n: F.linear(t, P[pre + n + ".weight"])
    q = lin(x, ".to_q")
    txt, img = context[:, :text_len], context[:, text_len:]
    B, N, C = q.shape
    d = C // heads
    sp = lambda t: t.reshape(t.shape[0], t.shape[1], heads, d).permute(0, 2, 1, 3)
    q = sp(q)

    def branch(kc, k, v):
        sim = torch.einsum("bhid,bhjd->bhij", q, sp(lin(kc, k))) * (d ** -0.5)
        return torch.einsum("bhij,bhjd->bhid", sim.softmax(dim=-1), sp(lin(kc, v))).permute(0, 2, 1, 3).reshape(B, N, C)
    o = branch(txt, ".to_k", ".to_v") + img_scale * branch(img, ".to_k_ip", ".to_v_ip")
    return F.linear(o, P[pre + ".to_out.0.weight"], P[pre + ".to_out.0.bias"])


def dc_spatial_transformer(x, context, P, pre, heads, text_len=77):
    """x [(b t), c, h, w], context [(b t), 77 + n, ctx] (SpatialTransformer.forward + BasicTransformerBlock._forward)"""
    b, c, h, w = x.shape
    x_in = x
    x = F.group_norm(x, 32, P[pre + ".norm.weight"], P[pre + ".norm.bias"], 1e-6)
    x = x.permute(0, 2, 3, 1).reshape(b, h * w, c)
    x = F.linear(x, P[pre + ".proj_in.weight"], P[pre + ".proj_in.bias"])
    bp = pre + ".transformer_blocks.0."
    ln = lambda t, n: F.layer_norm(t, (t.shape[-1],), P[bp + n + ".weight"], P[bp + n + ".bias"], 1e-5)
    x = U.cross_attention(ln(x, "norm1"), P, bp + "attn1", heads) + x
    x = dc_cross_attention(ln(x, "norm2"), P, bp + "attn2", heads, context, text_len) + x
    x = U.feed_forward(ln(x, "norm3"), P, bp + "ff") + x
    x = F.linear(x, P[pre + ".proj_out.weight"], P[pre + ".proj_out.bias"])
    return x.reshape(b, h, w, c).permute(0, 3, 1, 2) + x_in


def dc_expand_context(context, t, text_len=77):
    """openaimodel3d_dc.py:686-693: [B, 77 + t*16, C] -> [(B t), 77 + 16, C] with per-frame image tokens; else repeated over frames"""
    if context.shape[1] == text_len + t * IMG_TOKENS:
        txt = context[:, :text_len].repeat_interleave(t, dim=0)
        img = context[:, text_len:].reshape(context.shape[0] * t, IMG_TOKENS, context.shape[2])
        return torch.cat([txt, img], dim=1)
    return context.repeat_interleave(t, dim=0)


def dc_unet_forward(P, cfg, x, timesteps, context, fs=None, default_fs=10):
    """openaimodel3d_dc.UNetModel.forward (:676-735), eval mode.  x [B, 8, T, H, W] -> [B, C_out, T, H, W]"""
    dt = x.dtype
    mc = cfg.model_channels
    lin = lambda v, n: F.linear(v, P[n + ".weight"], P[n + ".bias"])
    b, _, t, hh, ww = x.shape
    emb = lin(F.silu(lin(U.timestep_embedding(timesteps, mc).to(dt), "time_embed.0")), "time_embed.2")
    if fs is None:
        fs = torch.full_like(timesteps, default_fs)
    emb = emb + lin(F.silu(lin(U.timestep_embedding(fs, mc).to(dt), "fps_embedding.0")), "fps_embedding.2")
    ctx = dc_expand_context(context, t, cfg.text_context_len)
    emb = emb.repeat_interleave(t, dim=0)
    h = x.permute(0, 2, 1, 3, 4).reshape(b * t, -1, hh, ww)

    def run(layers, h):
        for layer in layers:
            kind, pre, info = layer
            if kind == "st":
                h = dc_spatial_transformer(h, ctx, P, pre, info["heads"], cfg.text_context_len)
            else:
                h = U._run_block([layer], h, emb, ctx, b, P, cfg)
        return h
    st = U.structure(cfg)
    hs = []
    for i, blk in enumerate(st["input"]):
        h = run(blk, h)
        if i == 0 and st["init_attn"] is not None:
            h = run([st["init_attn"]], h)
        hs.append(h)
    h = run(st["middle"], h)
    for blk in st["output"]:
        h = run(blk, torch.cat([h, hs.pop()], dim=1))
    h = U.group_norm32(h, P["out.0.weight"], P["out.0.bias"])
    y = F.conv2d(F.silu(h), P["out.2.weight"], P["out.2.bias"], padding=1)
    return y.reshape(b, t, -1, hh, ww).permute(0, 2, 1, 3, 4)


# ---------------------------------------------------------------------------------------------------------------------
# Resampler (lvdm/modules/encoders/ip_resampler.py:65-152): PerceiverAttention + FeedForward layers over learned queries
# ---------------------------------------------------------------------------------------------------------------------
RS_TINY = dict(dim=128, depth=2, dim_head=64, heads=2, num_queries=4, embedding_dim=64, output_dim=64, ff_mult=2, video_length=4)


def rs_param_shapes(c):
    """state_dict keys of the reference Resampler(**c) in registration order"""
    n_lat = c["num_queries"] * (c["video_length"] or 1)
    inner = c["heads"] * c["dim_head"]
    sh = {"latents": (1, n_lat, c["dim"]), "proj_in.weight": (c["dim"], c["embedding_dim"]), "proj_in.bias": (c["dim"],),
          "proj_out.weight": (c["output_dim"], c["dim"]), "proj_out.bias": (c["output_dim"],),
          "norm_out.weight": (c["output_dim"],), "norm_out.bias": (c["output_dim"],)}
    for i in range(c["depth"]):
        a, f = f"layers.{i}.0.", f"layers.{i}.1."
        for n in ("norm1", "norm2"):
            sh[a + n + ".weight"] = (c["dim"],); sh[a + n + ".bias"] = (c["dim"],)
        sh[a + "to_q.weight"] = (inner, c["dim"]); sh[a + "to_kv.weight"] = (2 * inner, c["dim"]); sh[a + "to_out.weight"] = (c["dim"], inner)
        sh[f + "0.weight"] = (c["dim"],); sh[f + "0.bias"] = (c["dim"],)
        sh[f + "1.weight"] = (c["ff_mult"] * c["dim"], c["dim"]); sh[f + "3.weight"] = (c["dim"], c["ff_mult"] * c["dim"])
    return sh


def rs_init_params(c, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, s in rs_param_shapes(c).items():
        if k == "latents":
            w = torch.randn(s, generator=g) / math.sqrt(s[-1])
        elif len(s) == 1:
            w = torch.randn(s, generator=g) * 0.1 + (1.0 if k.endswith("weight") else 0.0)
        else:
            w = torch.randn(s, generator=g) * (0.7 / math.sqrt(s[1]))
        out[k] = w.to(dtype)
    return out


def rs_forward(P, c, x):
    """Resampler.forward: x [B, n1, embedding_dim] -> [B, num_queries * video_length, output_dim]"""
    H = c["heads"]
    ln = lambda t, n: F.layer_norm(t, (t.shape[-1],), P[n + ".weight"], P[n + ".bias"], 1e-5)
    lat = P["latents"].repeat(x.shape[0], 1, 1)
    x = F.linear(x, P["proj_in.weight"], P["proj_in.bias"])
    sp = lambda t: t.reshape(t.shape[0], t.shape[1], H, -1).permute(0, 2, 1, 3)
    for i in range(c["depth"]):
        a, f = f"layers.{i}.0.", f"layers.{i}.1."
        xn, l2 = ln(x, a + "norm1"), ln(lat, a + "norm2")
        q = sp(F.linear(l2, P[a + "to_q.weight"]))
        k, v = F.linear(torch.cat([xn, l2], dim=1), P[a + "to_kv.weight"]).chunk(2, dim=-1)
        w = torch.einsum("bhid,bhjd->bhij", q, sp(k)) * (c["dim_head"] ** -0.5)
        o = torch.einsum("bhij,bhjd->bhid", w.softmax(-1), sp(v)).permute(0, 2, 1, 3).reshape(lat.shape[0], lat.shape[1], -1)
        lat = F.linear(o, P[a + "to_out.weight"]) + lat
        lat = F.linear(F.gelu(F.linear(ln(lat, f + "0"), P[f + "1.weight"])), P[f + "3.weight"]) + lat
    return ln(F.linear(lat, P["proj_out.weight"], P["proj_out.bias"]), "norm_out")


RS_FLOW = dict(RS_TINY, num_queries=IMG_TOKENS)          # 16 queries per frame x 4 frames: the tiny UNet's per-frame image context


def dc_flow_loss(Pu, cfg, Pr, rcfg, z, context, image_tokens, t, noise, fs, cond_frame_index, alphas_cumprod, scale_arr, round_bf16=True,
                 model_dtype=None):
    """LatentVisualDiffusionFlow's deterministic core (ddpm3d.py:1311-1480 get_batch_input + :787-848 p_losses, parameterization v, use_scale,
    conditioning_key hybrid): Resampler -> [text | image] context; input = [q_sample(z * scale_t) | cond-frame latent repeated over time].
    model_dtype: the dtype the two networks run in (default: z's); the schedule arithmetic, the target and the loss stay in z's dtype, as the
    device keeps them in fp32 around its bf16 networks"""
    md = model_dtype or z.dtype
    rb = (lambda v: v.to(torch.bfloat16).to(md)) if round_bf16 else (lambda v: v.to(md))          # the device hands these to the UNet in bf16
    ctx = torch.cat([context.to(md), rb(rs_forward(Pr, rcfg, image_tokens.to(md)))], dim=1)
    T = z.shape[2]
    cond = z[:, :, cond_frame_index:cond_frame_index + 1].expand(-1, -1, T, -1, -1)
    x0 = z * scale_arr[t].view(-1, 1, 1, 1, 1).to(z.dtype)
    sa = alphas_cumprod[t].sqrt().float().to(z.dtype).view(-1, 1, 1, 1, 1)
    sb = (1 - alphas_cumprod[t]).sqrt().float().to(z.dtype).view(-1, 1, 1, 1, 1)
    x_in = torch.cat([rb(sa * x0 + sb * noise), rb(cond)], dim=1)
    out = dc_unet_forward(Pu, cfg, x_in, t, ctx, fs=fs).to(z.dtype)
    target = sa * noise - sb * x0
    return ((out - target) ** 2).mean(dim=(1, 2, 3, 4)).mean()


def dc_res_block_train(x, silu_emb, P, pre, batch_size, masks, p_drop):
    """ResBlock._forward in TRAIN mode with dropout p (openaimodel3d_dc.py:186-192: out_layers = GroupNorm, SiLU, Dropout(p), conv) followed by
    the TemporalConvBlock with its own three dropouts.  x [(b t), c, h, w]; silu_emb = SiLU(emb) [(b t), 4*mc];
    masks: {pre + ".out_layers.2": keep [(b t), c, h, w], pre + ".temopral_conv.conv{2,3,4}": keep [b, c, t, h, w]}"""
    h = U.group_norm32(x, P[pre + ".in_layers.0.weight"], P[pre + ".in_layers.0.bias"])
    h = F.conv2d(F.silu(h), P[pre + ".in_layers.2.weight"], P[pre + ".in_layers.2.bias"], padding=1)
    h = h + F.linear(silu_emb, P[pre + ".emb_layers.1.weight"], P[pre + ".emb_layers.1.bias"])[:, :, None, None]
    h = F.silu(U.group_norm32(h, P[pre + ".out_layers.0.weight"], P[pre + ".out_layers.0.bias"]))
    h = h * masks[pre + ".out_layers.2"].to(h.dtype) / (1.0 - p_drop)
    h = F.conv2d(h, P[pre + ".out_layers.3.weight"], P[pre + ".out_layers.3.bias"], padding=1)
    if (pre + ".skip_connection.weight") in P:
        x = F.conv2d(x, P[pre + ".skip_connection.weight"], P[pre + ".skip_connection.bias"])
    h = x + h
    bt, c, hh, ww = h.shape
    h5 = h.reshape(batch_size, bt // batch_size, c, hh, ww).permute(0, 2, 1, 3, 4)
    h5 = U.temporal_conv_block(h5, P, pre + ".temopral_conv", masks)
    return h5.permute(0, 2, 1, 3, 4).reshape(bt, c, hh, ww)
