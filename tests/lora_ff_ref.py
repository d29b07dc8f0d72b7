"""TEST INFRASTRUCTURE: the CPU restatement of the CogVideoX block with LoRA on the feed-forward pair ff.net.0.proj / ff.net.2
(DESIGN 3 "Feed-forward targets").

The oracle's dit_block runs the feed-forward with plain F.linear, so the block is restated here with an adapter-aware Linear on all six
block Linears (project code of the tests; the oracle file is not edited and stays the reference for everything but the two calls that
differ: ``dit_forward`` runs with ``cogvideox_oracle.dit_block`` replaced by ``block`` below through pytest's monkeypatch).  At p = 0 the
restatement must equal the oracle's block on merged weights W + s B A (tests/test_lora_ff_cpu.py).

lora_dropout: the mask of an adapter site over its Linear's input [M = B * S, in_features] is ``oracle/philox.py:
dropout_keep_mask(M, in_features, p, seed, offset = site << 36)``; the attention sites are 4 * layer + {0, 1, 2, 3} as before and the
feed-forward sites follow all of them: 4 * L + 2 * layer + {0, 1} for ff.net.0.proj, ff.net.2.

Three deliberately wrong references show that a comparison can tell them from the right one:
  "attn_sites":    the feed-forward adapters use the masks of sites 4 * layer + {0, 1} (to_q's and to_k's);
  "no_scale":      the feed-forward adapters lack the factor 1 / (1 - p);
  "dgelu_outside": in the backward of ff.net.2 the adapter's input-gradient correction is added after the factor gelu'(u) instead of
                   before it: du = gelu'(u) (x) (dY W2) + keep (x) (dT2 A2) / (1 - p).
"""
import re

import torch
import torch.nn.functional as F

import cogvideox_oracle as O
from lora_dropout_ref import SEED, flat, keep_mask, overall, rope_tables, tiny_inputs       # noqa: F401  (re-exported for the tests)

TARGETS = ("to_q", "to_k", "to_v", "to_out.0", "ff.net.0.proj", "ff.net.2")
PATHS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "ff.net.0.proj", "ff.net.2")
VARIANTS = ("right", "attn_sites", "no_scale", "dgelu_outside")
WRONG_SCALING = 4.0        # alpha / r of the runs that must reject the wrong variants: large enough for ff.net.2's dX correction to show
_NAME = re.compile(r"transformer_blocks\.(\d+)\.(.+)$")


def param_name(layer: int, kind: str, j: int) -> str:
    return f"transformer_blocks.{layer}.{PATHS[j]}.lora_{kind}.default.weight"


def is_ff(name: str) -> bool:
    return ".ff.net." in name


def site_of(name: str, L: int, variant: str = "right") -> int:
    m = _NAME.search(name)
    layer, j = int(m.group(1)), PATHS.index(m.group(2))
    if j < 4:
        return 4 * layer + j
    return 4 * layer + (j - 4) if variant == "attn_sites" else 4 * L + 2 * layer + (j - 4)


def make_lin(p: float, seed: int, L: int, variant: str = "right"):
    """lin(x, P, name, lora, lora_scale, x_lora=None): W x + b + s B A drop(x_lora or x), peft's Linear with the engine's masks"""
    assert variant in VARIANTS

    def lin(x, P, name, lora=None, lora_scale=0.25, x_lora=None):
        y = F.linear(x, P[name + ".weight"], P[name + ".bias"])
        if lora is not None and (name + ".lora_A.default.weight") in lora:
            A, Bm = lora[name + ".lora_A.default.weight"], lora[name + ".lora_B.default.weight"]
            xl = x if x_lora is None else x_lora
            if p > 0:
                k = xl.shape[-1]
                keep = keep_mask(xl.numel() // k, k, p, seed, site_of(name, L, variant)).view(xl.shape).to(xl.dtype)   # rows m = b * S + s
                xl = xl * keep * (1.0 if (variant == "no_scale" and is_ff(name)) else 1.0 / (1.0 - p))
            y = y + lora_scale * F.linear(F.linear(xl, A), Bm)
        return y
    return lin


def make_block(p: float = 0.0, seed: int = 0, variant: str = "right"):
    """a replacement for cogvideox_oracle.dit_block with adapters on all six Linears"""
    def block(h_txt, h_vid, emb, P, prefix, cfg, lora=None, lora_scale=0.25, taps=None, rope=None):
        lin = make_lin(p, seed, cfg.num_layers, variant)
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
        g = O.gelu_tanh(u)
        # "dgelu_outside": the adapter reads gelu(u)'s value but hands its input gradient to u without the factor gelu'(u)
        g_lora = g.detach() + (u - u.detach()) if variant == "dgelu_outside" else None
        f = lin(g, P, prefix + "ff.net.2", lora, lora_scale, x_lora=g_lora)
        h_vid = h_vid + gate * f[:, St:]
        h_txt = h_txt + egate * f[:, :St]
        return h_txt, h_vid
    return block


def oracle_params(model, st, dtype=torch.float64):
    """selfcheck.oracle_params for a state with feed-forward adapters: bf16-rounded weights in the oracle's key layout"""
    P = {k.replace(".base_layer", ""): v.detach().float().cpu().to(dtype) for k, v in model.state_dict().items() if "lora" not in k}
    Lo = {param_name(layer, kind, j): p.detach().to(torch.bfloat16).float().cpu().to(dtype)
          for p, (layer, kind, j) in zip(st.params, st._index)}
    return P, Lo


def device_grads(st):
    return {param_name(layer, kind, j): st.view(st.grad, layer, kind, j).detach().cpu().double().clone() for (layer, kind, j) in st._index}


def reference_step(monkeypatch, cfg, model, st, noisy, x0, text, t, p, seed, variant="right", rope_tabs=None):
    """fp64 loss and {adapter parameter name: gradient} of one training step with the restated block under lora_dropout (p, seed).
    noisy: the noised latents the device saw, as an fp64 CPU tensor."""
    P, Lo = oracle_params(model, st)
    for v in Lo.values():
        v.requires_grad_(True)
    abar = O.alphas_cumprod_cogvideox()
    with monkeypatch.context() as mp:
        mp.setattr(O, "dit_block", make_block(p, seed, variant))
        out_ref = O.dit_forward(P, cfg, noisy, text.double(), t, Lo, st.scaling,
                                image_rotary_emb=None if rope_tabs is None else (rope_tabs[0].double(), rope_tabs[1].double()))
    pred = O.get_velocity(out_ref, noisy, t, abar)
    wref = (1.0 / (1.0 - abar[t])).view(-1, 1, 1, 1, 1)
    loss_ref = torch.mean((wref * (pred - x0.double()) ** 2).reshape(x0.shape[0], -1), dim=1).mean()
    loss_ref.backward()
    return loss_ref.item(), {k: v.grad.detach().clone() for k, v in Lo.items()}, out_ref.detach()


def ff_names(grads):
    return [k for k in grads if is_ff(k)]


def build_tiny(device, targets=TARGETS, lora_r=4, lora_b_random=True, p=0.0, layers=2, seed=0, scaling=0.25, **cfg_kw):
    """selfcheck.build_tiny with a target list, lora_dropout and lora_alpha = scaling * r: B ~ 0.02 randn as there"""
    from selfcheck import CFG_KEYS
    from vt355.dit import CogVideoXTransformer3DModel
    from vt355.lora import LoraConfig, get_peft_model
    cfg = O.tiny_config(num_layers=layers, num_attention_heads=2, **cfg_kw)
    model = CogVideoXTransformer3DModel(**{k: getattr(cfg, k) for k in CFG_KEYS}).init_weights(seed).to(device)
    model.requires_grad_(False)
    # the adapter_config node of a CogVideoX recipe (cogvideo2b.yaml's, with the longer target list), through the config loader
    from vt355.config import instantiate_from_config
    lcfg = instantiate_from_config({"target": "peft.LoraConfig", "params": {
        "r": lora_r, "lora_alpha": lora_r * scaling, "init_lora_weights": True, "target_modules": list(targets), "lora_dropout": p}})
    assert isinstance(lcfg, LoraConfig)
    peft = get_peft_model(model, lcfg)
    st = peft._lora_state
    if lora_b_random:
        g = torch.Generator().manual_seed(seed + 7)
        with torch.no_grad():
            for prm, (layer, kind, j) in zip(st.params, st._index):
                if kind == "B":
                    prm.copy_((torch.randn(prm.shape, generator=g) * 0.02).to(prm.device))
        st.mark_changed()
    return cfg, model, peft, st
