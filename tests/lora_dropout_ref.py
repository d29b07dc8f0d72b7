"""TEST INFRASTRUCTURE: the CPU restatement of lora_dropout for the CogVideoX DiT (DESIGN 3 "LoRA dropout").

peft 0.12's Linear.forward is ``result + lora_B(lora_A(dropout(x))) * scaling`` with one nn.Dropout(p) per adapted Linear.  The engine
takes its masks from Philox instead of torch's generator; the mask of adapter site s = 4 * layer + j (j = 0..3 for to_q, to_k, to_v,
to_out.0) over the adapter input [M = B * S, d] is ``oracle/philox.py: dropout_keep_mask(M, d, p, seed, offset = s << 36)``.  The fp64
reference is the CogVideoX oracle with ``cogvideox_oracle._lin`` patched (pytest's monkeypatch; the oracle file is not edited) to apply
``x * mask_s / (1 - p)`` in front of lora_A.

Three deliberately wrong references show that the comparison can tell them from the right one:
  "shared_qkv": to_k and to_v use to_q's mask (one mask for the fused projection);
  "next_site":  every adapter uses the mask of site s + 1;
  "no_scale":   the factor 1 / (1 - p) is missing.
"""
import functools
import re

import numpy as np
import torch
import torch.nn.functional as F

import cogvideox_oracle as O
import philox

TARGETS = ("to_q", "to_k", "to_v", "to_out.0")
VARIANTS = ("right", "shared_qkv", "next_site", "no_scale")
SEED = 0x2F3C5A7E9B1D4C68 & (2 ** 62 - 1)          # both key words non-zero
SITE0 = 116                                        # layer 29: (116 << 36) >> 32 = 0x740, the counter's upper word is non-zero
_NAME = re.compile(r"transformer_blocks\.(\d+)\.attn1\.(to_q|to_k|to_v|to_out\.0)$")


def site_of(name: str) -> int:
    m = _NAME.search(name)
    assert m, name
    return 4 * int(m.group(1)) + TARGETS.index(m.group(2))


@functools.lru_cache(maxsize=64)
def _mask_np(M, d, p, seed, site):
    return philox.dropout_keep_mask(M, d, p, seed, offset=site << 36)


def keep_mask(M: int, d: int, p: float, seed: int, site: int) -> torch.Tensor:
    """fp64 0/1 [M, d]"""
    return torch.from_numpy(_mask_np(M, d, float(p), int(seed), int(site)).astype(np.float64))


def dropped_lin(p: float, seed: int, variant: str = "right"):
    """a replacement for cogvideox_oracle._lin that applies lora_dropout as the engine defines it (or one of the wrong variants)"""
    assert variant in VARIANTS

    def _lin(x, P, name, lora=None, lora_scale=0.25):
        y = F.linear(x, P[name + ".weight"], P[name + ".bias"])
        if lora is not None and (name + ".lora_A.default.weight") in lora:
            A = lora[name + ".lora_A.default.weight"]
            Bm = lora[name + ".lora_B.default.weight"]
            s = site_of(name)
            if variant == "shared_qkv" and s % 4 < 3:
                s -= s % 4
            if variant == "next_site":
                s += 1
            d = x.shape[-1]
            keep = keep_mask(x.numel() // d, d, p, seed, s).view(x.shape).to(x.dtype)      # rows in the engine's order: m = b * S + s
            xd = x * keep * (1.0 if variant == "no_scale" else 1.0 / (1.0 - p))
            y = y + lora_scale * F.linear(F.linear(xd, A), Bm)
        return y
    return _lin


def patch_oracle(monkeypatch, p: float, seed: int, variant: str = "right"):
    monkeypatch.setattr(O, "_lin", dropped_lin(p, seed, variant))


# ---------------------------------------------------------------------------------------------------------------- the tiny training step
def tiny_inputs(cfg, B=2):
    """the inputs of selfcheck.tiny_train_step_check"""
    g = torch.Generator().manual_seed(123)
    Fr = (cfg.sample_frames - 1) // 4 + 1
    x0 = torch.randn(B, Fr, 16, cfg.sample_height, cfg.sample_width, generator=g)
    text = (torch.randn(B, cfg.max_text_seq_length, cfg.text_embed_dim, generator=g) * 0.5).to(torch.bfloat16)
    noise = torch.randn(x0.shape, generator=g)
    t = torch.tensor([200, 800][:B])
    return x0, text, noise, t


def rope_tables(cfg, rope: bool):
    if not rope:
        return None
    Fr = (cfg.sample_frames - 1) // 4 + 1
    grid = (cfg.sample_height // 2, cfg.sample_width // 2)
    return O.rope_3d_tables(64, O.resize_crop_region_for_grid(grid, (3, 4)), grid, Fr)


def reference_step(monkeypatch, cfg, model, st, noisy, x0, text, t, p, seed, variant="right", rope_tabs=None):
    """fp64 loss and {adapter parameter name: gradient} of one training step under lora_dropout (p, seed); p == 0 leaves the oracle as it is.
    noisy: the noised latents the device saw, as an fp64 CPU tensor."""
    from selfcheck import oracle_params
    P, Lo = oracle_params(model, st, torch.float64)
    for v in Lo.values():
        v.requires_grad_(True)
    abar = O.alphas_cumprod_cogvideox()
    with monkeypatch.context() as mp:
        if p > 0:
            patch_oracle(mp, p, seed, variant)
        out_ref = O.dit_forward(P, cfg, noisy, text.double(), t, Lo, st.scaling,
                                image_rotary_emb=None if rope_tabs is None else (rope_tabs[0].double(), rope_tabs[1].double()))
    pred = O.get_velocity(out_ref, noisy, t, abar)
    wref = (1.0 / (1.0 - abar[t])).view(-1, 1, 1, 1, 1)
    loss_ref = torch.mean((wref * (pred - x0.double()) ** 2).reshape(x0.shape[0], -1), dim=1).mean()
    loss_ref.backward()
    return loss_ref.item(), {k: v.grad.detach().clone() for k, v in Lo.items()}


def flat(grads, names=None):
    return torch.cat([grads[k].reshape(-1) for k in (names or grads)])


def overall(gdev, gref):
    """(rel-L2, cosine) over all adapter gradients concatenated: the two figures tiny_train_step_check bounds"""
    a, b = gdev.double(), gref.double()
    return ((a - b).norm() / b.norm()).item(), F.cosine_similarity(a, b, dim=0).item()
