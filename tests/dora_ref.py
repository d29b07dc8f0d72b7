"""TEST INFRASTRUCTURE: the CPU restatement of the CogVideoX block with DoRA adapters (LoraConfig.use_dora, DESIGN 3 "DoRA") on any of
the six block Linears, built like tests/lora_ff_ref.py: ``dit_forward`` runs with ``cogvideox_oracle.dit_block`` replaced by ``block``
below through pytest's monkeypatch; the oracle file is not edited.

The adapted Linear is peft 0.12's DoraLinearLayer written literally (no dropout):

    norm = || W + s B A ||_2 per output row, DETACHED          c = m / norm
    y    = base(x) + (c - 1) * F.linear(x, W) + c * s * B(A(x))          (base(x) = W x + b: the bias is not scaled)

which must equal the oracle's plain block on the merged weights diag(c) (W + s B A) (tests/test_dora_cpu.py).

Three deliberately wrong references show that a comparison can tell them from the right one:
  "norm_attached": the gradient flows through the norm (dA and dB gain the term through c);
  "bias_scaled":   y = c (x) (W x + s B A x + b);
  "norm_of_w":     the norm ignores s B A: c = m / ||W||.
"""
import torch
import torch.nn.functional as F

import cogvideox_oracle as O
from lora_dropout_ref import flat, overall, rope_tables, tiny_inputs       # noqa: F401  (re-exported for the tests)

TARGETS = ("to_q", "to_k", "to_v", "to_out.0", "ff.net.0.proj", "ff.net.2")
PATHS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "ff.net.0.proj", "ff.net.2")
VARIANTS = ("right", "norm_attached", "bias_scaled", "norm_of_w")
KIND = {"A": "lora_A", "B": "lora_B", "M": "lora_magnitude_vector"}
# The inputs of the step tests.  tests/test_dora_cpu.py shows that every wrong variant leaves the step's bars at them.  At the siblings'
# alpha / r = 0.25 and B ~ 0.02 randn, s B A is 0.1 % of a row norm: "norm_of_w" moves the gradients by 0.3 % and "norm_attached" the
# adapter group by 7.6 % (measured at r = 4), too close to the 6 % bar; so the perturbations were raised, not the bars: s B A about as
# large as W at every rank, and larger biases so that "bias_scaled" shows at every rank too.
STEP_SCALING = 4.0         # alpha / r
STEP_B_GAIN = 0.1          # B ~ STEP_B_GAIN / sqrt(r) * randn: the size of B A does not depend on the rank
STEP_M_STD = 0.1           # m = ||W + s B A|| * (1 + STEP_M_STD * randn)
STEP_BIAS_GAIN = 10.0      # the biases of the six block Linears are multiplied by this


def param_name(layer: int, kind: str, j: int) -> str:
    return f"transformer_blocks.{layer}.{PATHS[j]}.{KIND[kind]}.default.weight"


def is_mag(name: str) -> bool:
    return "lora_magnitude_vector" in name


def mag_names(grads):
    return [k for k in grads if is_mag(k)]


def adapter_names(grads):
    return [k for k in grads if not is_mag(k)]


def make_lin(variant: str = "right"):
    """lin(x, P, name, lora, lora_scale): peft's DoRA Linear (a Linear without a magnitude in ``lora`` is a plain LoRA or a plain Linear)"""
    assert variant in VARIANTS

    def lin(x, P, name, lora=None, lora_scale=0.25):
        W, b = P[name + ".weight"], P[name + ".bias"]
        base = F.linear(x, W, b)
        if lora is None or (name + ".lora_A.default.weight") not in lora:
            return base
        A, Bm = lora[name + ".lora_A.default.weight"], lora[name + ".lora_B.default.weight"]
        up = lora_scale * F.linear(F.linear(x, A), Bm)
        mk = name + ".lora_magnitude_vector.default.weight"
        if mk not in lora:
            return base + up
        m = lora[mk]
        norm = torch.linalg.norm(W if variant == "norm_of_w" else W + lora_scale * Bm @ A, dim=1)
        if variant != "norm_attached":
            norm = norm.detach()
        c = m / norm
        if variant == "bias_scaled":
            return c * (base + up)
        return base + (c - 1) * F.linear(x, W) + c * up
    return lin


def make_block(variant: str = "right"):
    """a replacement for cogvideox_oracle.dit_block with (DoRA) adapters on all six Linears"""
    lin = make_lin(variant)

    def block(h_txt, h_vid, emb, P, prefix, cfg, lora=None, lora_scale=0.25, taps=None, rope=None):
        d, H, hd = cfg.inner_dim, cfg.num_attention_heads, cfg.attention_head_dim
        St, B = h_txt.shape[1], h_vid.shape[0]

        def ln_zero(name, hv, ht):
            mod = F.linear(F.silu(emb), P[prefix + name + ".linear.weight"], P[prefix + name + ".linear.bias"])
            shift, scale, gate, eshift, escale, egate = mod.chunk(6, dim=1)
            w, b = P[prefix + name + ".norm.weight"], P[prefix + name + ".norm.bias"]
            nv = F.layer_norm(hv, (d,), w, b, cfg.norm_eps) * (1 + scale)[:, None] + shift[:, None]
            nt = F.layer_norm(ht, (d,), w, b, cfg.norm_eps) * (1 + escale)[:, None] + eshift[:, None]
            return nv, nt, gate[:, None], egate[:, None]

        nv, nt, gate, egate = ln_zero("norm1", h_vid, h_txt)
        x = torch.cat([nt, nv], dim=1)                                   # text first
        a = prefix + "attn1."
        q, k, v = (lin(x, P, a + n, lora, lora_scale).view(B, -1, H, hd).transpose(1, 2) for n in ("to_q", "to_k", "to_v"))
        q = F.layer_norm(q, (hd,), P[a + "norm_q.weight"], P[a + "norm_q.bias"], cfg.qk_norm_eps)
        k = F.layer_norm(k, (hd,), P[a + "norm_k.weight"], P[a + "norm_k.bias"], cfg.qk_norm_eps)
        if rope is not None:
            q = torch.cat([q[:, :, :St], O.apply_rope(q[:, :, St:], *rope)], dim=2)
            k = torch.cat([k[:, :, :St], O.apply_rope(k[:, :, St:], *rope)], dim=2)
        o = F.scaled_dot_product_attention(q, k, v, dropout_p=0.0, is_causal=False).transpose(1, 2).reshape(B, -1, d)
        o = lin(o, P, a + "to_out.0", lora, lora_scale)
        h_vid = h_vid + gate * o[:, St:]
        h_txt = h_txt + egate * o[:, :St]

        nv, nt, gate, egate = ln_zero("norm2", h_vid, h_txt)
        x = torch.cat([nt, nv], dim=1)
        u = lin(x, P, prefix + "ff.net.0.proj", lora, lora_scale)
        f = lin(O.gelu_tanh(u), P, prefix + "ff.net.2", lora, lora_scale)
        h_vid = h_vid + gate * f[:, St:]
        h_txt = h_txt + egate * f[:, :St]
        return h_txt, h_vid
    return block


def oracle_params(model, st, dtype=torch.float64):
    """base weights and A / B as the products see them (bf16-rounded), the magnitudes as their fp32 masters (c is formed from those)"""
    P = {k.replace(".base_layer", ""): v.detach().float().cpu().to(dtype) for k, v in model.state_dict().items() if "lora" not in k}
    Lo = {}
    for p, (layer, kind, j) in zip(st.params, st._index):
        v = p.detach() if kind == "M" else p.detach().to(torch.bfloat16)
        Lo[param_name(layer, kind, j)] = v.float().cpu().to(dtype)
    return P, Lo


def device_grads(st):
    return {param_name(layer, kind, j): st.view(st.grad, layer, kind, j).detach().cpu().double().clone() for (layer, kind, j) in st._index}


def reference_step(monkeypatch, cfg, model, st, noisy, x0, text, t, variant="right", rope_tabs=None, params=None):
    """fp64 loss, {parameter name: gradient} and prediction of one training step with the restated block.  noisy: the noised latents the
    device saw, as an fp64 CPU tensor.  params: (P, Lo) to evaluate at (default: the model's current ones)."""
    P, Lo = oracle_params(model, st) if params is None else params
    for v in Lo.values():
        v.requires_grad_(True)
    abar = O.alphas_cumprod_cogvideox()
    with monkeypatch.context() as mp:
        mp.setattr(O, "dit_block", make_block(variant))
        out_ref = O.dit_forward(P, cfg, noisy, text.double(), t, Lo, st.scaling,
                                image_rotary_emb=None if rope_tabs is None else (rope_tabs[0].double(), rope_tabs[1].double()))
    pred = O.get_velocity(out_ref, noisy, t, abar)
    wref = (1.0 / (1.0 - abar[t])).view(-1, 1, 1, 1, 1)
    loss_ref = torch.mean((wref * (pred - x0.double()) ** 2).reshape(x0.shape[0], -1), dim=1).mean()
    loss_ref.backward()
    return loss_ref.item(), {k: v.grad.detach().clone() for k, v in Lo.items()}, out_ref.detach()


def build_tiny(device, targets=TARGETS, lora_r=4, use_dora=True, b_std=None, m_std=STEP_M_STD, bias_gain=STEP_BIAS_GAIN, layers=2,
               seed=0, scaling=STEP_SCALING, **cfg_kw):
    """the tiny model of selfcheck.build_tiny with DoRA adapters from the recipe's adapter_config node: B ~ b_std randn (None: STEP_B_GAIN
    / sqrt(r); 0: peft's init),
    the magnitudes re-initialised at those adapters and then perturbed by (1 + m_std randn) so that c != 1 (m_std = 0: untouched), the
    biases of the block Linears times bias_gain"""
    from selfcheck import CFG_KEYS
    from vt355.config import instantiate_from_config
    from vt355.dit import CogVideoXTransformer3DModel
    from vt355.lora import LoraConfig, get_peft_model
    b_std = STEP_B_GAIN / lora_r ** 0.5 if b_std is None else b_std
    cfg = O.tiny_config(num_layers=layers, num_attention_heads=2, **cfg_kw)
    model = CogVideoXTransformer3DModel(**{k: getattr(cfg, k) for k in CFG_KEYS}).init_weights(seed)
    if bias_gain != 1.0:
        with torch.no_grad():
            for n, p in model.named_parameters():
                if n.startswith("transformer_blocks.") and n.endswith(".bias") and any(n.endswith(pth + ".bias") for pth in PATHS):
                    p.mul_(bias_gain)
    model = model.to(device)
    model.requires_grad_(False)
    lcfg = instantiate_from_config({"target": "peft.LoraConfig", "params": {
        "r": lora_r, "lora_alpha": lora_r * scaling, "init_lora_weights": True, "target_modules": list(targets), "use_dora": use_dora}})
    assert isinstance(lcfg, LoraConfig)
    peft = get_peft_model(model, lcfg)
    st = peft._lora_state
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        if b_std:
            for prm, (layer, kind, j) in zip(st.params, st._index):
                if kind == "B":
                    prm.copy_((torch.randn(prm.shape, generator=g) * b_std).to(prm.device))
            if use_dora:
                st.init_magnitudes(model)
        if use_dora and m_std:
            for prm, (layer, kind, j) in zip(st.params, st._index):
                if kind == "M":
                    prm.mul_((1.0 + m_std * torch.randn(prm.shape, generator=g)).to(prm.device))
    st.mark_changed()
    return cfg, model, peft, st
