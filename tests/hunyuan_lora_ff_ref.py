"""Reference side of the HunyuanVideo feed-forward LoRA targets (tests/test_hunyuan_lora_ff_cpu.py, tests/test_hunyuan_lora_ff_gpu.py):
the adapters folded into effective weights W + scaling B A on the rows of each adapted Linear, built from the adapter tensors with autograd,
so that oracle.hunyuan_oracle's double_block / single_block run unchanged and the adapter gradients come out of them -- the pattern of
_lora_effective in tests/test_hunyuan_lora_wide_gpu.py, extended by the four feed-forward sites."""
import os

import numpy as np
import torch

ATTN = ("to_q", "to_k", "to_v", "to_out.0")
FF = ("ff.net.0.proj", "ff.net.2", "proj_mlp", "proj_out")
ALL = ATTN + FF
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def attn_sites(targets, n_double=1, n_single=1):
    """{module: adapter tags} of the attention group, empty unless `targets` (None: the default) names it"""
    if targets is not None and not set(ATTN) <= set(targets):
        return {}
    s = {}
    for i in range(n_double):
        s[f"double_blocks.{i}.img_attn_qkv"] = ("q", "k", "v")
        s[f"double_blocks.{i}.img_attn_proj"] = ("",)
    for i in range(n_single):
        s[f"single_blocks.{i}.linear1"] = ("q", "k", "v")
    return s


def ff_sites(targets, D, M4, n_double=1, n_single=1):
    """[(target, module, tag, first weight row, out width, in width)] of the feed-forward sites `targets` names, in parameter order"""
    t = set(targets or ())
    s = []
    for i in range(n_double):
        if "ff.net.0.proj" in t:
            s.append(("ff.net.0.proj", f"double_blocks.{i}.img_mlp.fc1", "", 0, M4, D))
        if "ff.net.2" in t:
            s.append(("ff.net.2", f"double_blocks.{i}.img_mlp.fc2", "", 0, D, M4))
    for i in range(n_single):
        if "proj_mlp" in t:
            s.append(("proj_mlp", f"single_blocks.{i}.linear1", "mlp", 3 * D, M4, D))
        if "proj_out" in t:
            s.append(("proj_out", f"single_blocks.{i}.linear2", "", 0, D, D + M4))
    return s


def adapter_names(targets, D, M4, n_double=1, n_single=1):
    """the adapters' parameter names and shapes for rank-free bookkeeping: [(name of A, (in width), name of B, (out width))] in flat order"""
    out = []
    for mod, tags in attn_sites(targets, n_double, n_single).items():
        for t in tags:
            dot = "." + t if t else ""
            out.append((f"{mod}.lora_A{dot}.weight", D, f"{mod}.lora_B{dot}.weight", D))
    for _, mod, tag, _, N, K in ff_sites(targets, D, M4, n_double, n_single):
        dot = "." + tag if tag else ""
        out.append((f"{mod}.lora_A{dot}.weight", K, f"{mod}.lora_B{dot}.weight", N))
    return out


def init_adapters(targets, D, M4, r, seed=5, n_double=1, n_single=1):
    """random adapters (B non-zero) for the CPU tests, {name: fp32 tensor}"""
    gen = torch.Generator().manual_seed(seed)
    ad = {}
    for na, K, nb, N in adapter_names(targets, D, M4, n_double, n_single):
        ad[na] = torch.randn(r, K, generator=gen) * K ** -0.5
        ad[nb] = torch.randn(N, r, generator=gen) * 0.05
    return ad


def lora_effective(base, ad, targets, scaling, D, M4, n_double=1, n_single=1, scaling_of=None):
    """base with W + scaling B A on the rows of each adapted Linear, in the dtype of base / ad.  scaling_of: {target: scaling} for single
    targets (a mutant's knob)"""
    sc = lambda t: (scaling_of or {}).get(t, scaling)
    Pe = dict(base)
    for mod, tags in attn_sites(targets, n_double, n_single).items():
        w = Pe[mod + ".weight"].clone()
        for j, t in enumerate(tags):
            dot = "." + t if t else ""
            tgt = "to_out.0" if not t else "to_" + t
            w[j * D:(j + 1) * D] = w[j * D:(j + 1) * D] + sc(tgt) * ad[f"{mod}.lora_B{dot}.weight"] @ ad[f"{mod}.lora_A{dot}.weight"]
        Pe[mod + ".weight"] = w
    for tgt, mod, tag, row0, N, K in ff_sites(targets, D, M4, n_double, n_single):
        dot = "." + tag if tag else ""
        w = Pe[mod + ".weight"].clone()
        w[row0:row0 + N] = w[row0:row0 + N] + sc(tgt) * ad[f"{mod}.lora_B{dot}.weight"] @ ad[f"{mod}.lora_A{dot}.weight"]
        Pe[mod + ".weight"] = w
    return Pe


def golden():
    g = np.load(os.path.join(G, "hunyuan_blocks.npz"))
    return lambda k: torch.from_numpy(g[k])


def blocks_loss(HO, Pe, img, txt, vec, tv, cos, sin, gx, H):
    """(output, sum(output * gx)) of one double and one single block of the oracle on the parameters Pe, in Pe's dtype; the loss is taken in
    fp64 from an fp64 run and in fp32 from a bf16 run's bf16 output, as on the device"""
    io, to = HO.double_block(img, txt, vec, Pe, "double_blocks.0.", H, tv, cos, sin)
    xo = HO.single_block(torch.cat([io, to], 1), vec, Pe, "single_blocks.0.", H, txt.shape[1], tv, cos, sin)
    ld = torch.float64 if xo.dtype == torch.float64 else torch.float32
    return xo, (xo.to(ld) * gx.to(ld)).sum()
