"""Reference side of HunyuanVideo lora_dropout (tests/test_hunyuan_lora_dropout_cpu.py, tests/test_hunyuan_lora_dropout_gpu.py): the
blocks of oracle.hunyuan_oracle run with the module's ``F`` replaced by a shim (hunyuan_oracle.py itself is not edited) whose ``linear``
recognises an adapted weight by tensor identity and adds, on each adapter's output rows,

    s * B A (keep * x) / (1 - p)

with the adapter's own keep mask -- peft 0.12's one nn.Dropout in front of lora_A of each adapted Linear.  The masks are the engine's
(include/vt355.h "mask convention"): adapter site s = the adapter's position among the lora_A parameters, element (m_g, k) of the Linear's
input [M_g, K] (m_g the row of the UNSHARDED run: b L + l, image rows first) kept iff oracle/philox.py's
dropout_keep_mask(M_g, K, p, seed, offset = s << 36) says so.

Four deliberately wrong variants show that the bars of the tests tell right from wrong:
  shared_qkv   the q, k, v adapters of a fused projection share the q adapter's mask
  next_site    every adapter uses the mask of site s + 1
  no_scale     the factor 1 / (1 - p) is missing
  local_rows   the masks are keyed by the row of one rank's slice of a `world`-rank sequence-parallel run (image rows split into `world`
               contiguous parts, the text rows behind each part) instead of the unsharded row
"""
import contextlib

import numpy as np
import torch
import torch.nn.functional as TF

from hunyuan_lora_ff_ref import attn_sites, ff_sites

VARIANTS = ("right", "shared_qkv", "next_site", "no_scale", "local_rows")


def adapter_sites(targets, D, M4, n_double=1, n_single=1):
    """[(site, module, tag, first output row, out width, in width, joint)] in site order = parameter order of the lora_A entries: the
    attention group (q, k, v of a fused projection consecutive), then the feed-forward sites.  joint: the Linear sees [image; text] rows
    (single blocks), else the image rows"""
    out = []
    for mod, tags in attn_sites(targets, n_double, n_single).items():
        for j, t in enumerate(tags):
            out.append((len(out), mod, t, j * D, D, D, mod.startswith("single_blocks.")))
    for _, mod, tag, row0, N, K in ff_sites(targets, D, M4, n_double, n_single):
        out.append((len(out), mod, tag, row0, N, K, mod.startswith("single_blocks.")))
    return out


def keep_mask(rows, K, p, seed, site):
    """float64 [rows, K] keep mask of adapter site `site`; p is taken as the float32 the C ABI carries"""
    import philox
    return torch.from_numpy(philox.dropout_keep_mask(rows, K, float(np.float32(p)), seed, offset=site << 36).astype(np.float64))


def local_row_index(B, Li, Lt, joint, world):
    """index [B * L] of each unsharded row's position within its rank's local row space (the row a locally keyed mask would use)"""
    Lil = Li // world
    idx = []
    for b in range(B):
        for l in range(Li):
            idx.append(b * (Lil + (Lt if joint else 0)) + l % Lil)
        if joint:
            for t in range(Lt):
                idx.append(b * (Lil + Lt) + Lil + t)
    return torch.tensor(idx, dtype=torch.long)


class _Shim:
    """stands in for torch.nn.functional inside hunyuan_oracle: everything passes through but ``linear``"""

    def __init__(self, adapters_of, p, seed, variant, geometry):
        self.adapters_of, self.p, self.seed, self.variant, self.geometry = adapters_of, p, seed, variant, geometry
        self.hits = 0

    def __getattr__(self, name):
        return getattr(TF, name)

    def mask(self, site, q_site, rows, K, joint):
        v = self.variant
        s = q_site if v == "shared_qkv" else site + 1 if v == "next_site" else site
        if v == "local_rows":
            B, Li, Lt, world = self.geometry
            idx = local_row_index(B, Li, Lt, joint, world)
            assert idx.numel() == rows
            return keep_mask(int(idx.max()) + 1, K, self.p, self.seed, s)[idx]
        return keep_mask(rows, K, self.p, self.seed, s)

    def linear(self, x, w, b=None):
        y = TF.linear(x, w, b)
        for site, q_site, row0, N, A, Bm, scaling, joint in self.adapters_of.get(id(w), ()):
            self.hits += 1
            K = x.shape[-1]
            x2 = x.reshape(-1, K)
            xd = x2
            if self.p > 0:
                xd = x2 * self.mask(site, q_site, x2.shape[0], K, joint).to(x.dtype)
            t = xd @ A.t()
            if self.p > 0 and self.variant != "no_scale":
                t = t * (1.0 / (1.0 - float(np.float32(self.p))))
            d = (scaling * (t @ Bm.t())).reshape(*x.shape[:-1], N)
            y = y + TF.pad(d, (row0, y.shape[-1] - row0 - N))
        return y


@contextlib.contextmanager
def dropped_oracle(HO, base, ad, targets, scaling, D, M4, p, seed, variant="right", geometry=None, n_double=1, n_single=1):
    """inside: HO.double_block / HO.single_block on the parameters `base` apply the adapters `ad` under dropout p.  geometry =
    (B, Li, Lt, world) for the local_rows variant.  Yields the shim (shim.hits: adapter applications so far)"""
    assert variant in VARIANTS
    adapters_of = {}
    q_site = 0
    for site, mod, tag, row0, N, K, joint in adapter_sites(targets, D, M4, n_double, n_single):
        dot = "." + tag if tag else ""
        if tag in ("q", ""):
            q_site = site
        adapters_of.setdefault(id(base[mod + ".weight"]), []).append(
            (site, q_site if tag in ("q", "k", "v") else site, row0, N, ad[f"{mod}.lora_A{dot}.weight"], ad[f"{mod}.lora_B{dot}.weight"], scaling, joint))
    shim = _Shim(adapters_of, p, seed, variant, geometry)
    saved = HO.F
    HO.F = shim
    try:
        yield shim
    finally:
        HO.F = saved


def blocks_run(HO, P, img, txt, vec, tv, cos, sin, gx, H, n_double=1, n_single=1):
    """(output, sum(output * gx)) of n_double double and n_single single blocks of the oracle on the parameters P (hunyuan_lora_ff_ref's
    blocks_loss for any depth)"""
    io, to = img, txt
    for i in range(n_double):
        io, to = HO.double_block(io, to, vec, P, f"double_blocks.{i}.", H, tv, cos, sin)
    x = torch.cat([io, to], 1)
    for i in range(n_single):
        x = HO.single_block(x, vec, P, f"single_blocks.{i}.", H, txt.shape[1], tv, cos, sin)
    ld = torch.float64 if x.dtype == torch.float64 else torch.float32
    return x, (x.to(ld) * gx.to(ld)).sum()


def reference_step(HO, base, ad, targets, scaling, D, M4, H, inputs, p, seed, variant="right", dtype=torch.float64, world=2,
                   n_double=1, n_single=1):
    """one forward + backward of the dropped oracle in `dtype` (fp64: the reference; bf16: its restatement, every op rounding to bf16).
    inputs = (img, txt, vec, tv, cos, sin, dout) CPU tensors.  Returns dict(out, dimg, dtxt, grads {adapter name: gradient}, hits)"""
    img, txt, vec, tv, cos, sin, dout = inputs
    lp = dtype != torch.float64
    leaf = lambda t: t.detach().to(dtype).requires_grad_(True)
    b = {k: v.detach().to(dtype) for k, v in base.items()}
    a = {k: leaf(v) for k, v in ad.items()}
    ri, rt, rv = leaf(img), leaf(txt), leaf(vec)
    tab = (cos, sin) if lp else (cos.double(), sin.double())
    geo = (img.shape[0], img.shape[1], txt.shape[1], world)
    with dropped_oracle(HO, b, a, targets, scaling, D, M4, p, seed, variant, geo, n_double, n_single) as shim:
        xo, loss = blocks_run(HO, b, ri, rt, rv, tv, tab[0], tab[1], dout, H, n_double, n_single)
    loss.backward()
    return dict(out=xo.detach(), dimg=ri.grad, dtxt=rt.grad, grads={k: v.grad for k, v in a.items()}, hits=shim.hits)


def verdict(got, ref, noisy, valid, Li):
    """the train-step bars (test_hunyuan_lora_ff_gpu._train_step_vs_oracle's) on a result `got` against the fp64 `ref`, the bf16
    restatement `noisy` giving the gradient floor: forward 1e-2 over the valid rows, d(img) / d(txt) 3e-2, every adapter gradient under
    parity.floor_bars(cosine 0.98, cap 0.2), overall under 1.5 x the floor.  got / ref / noisy: reference_step's dicts.  Returns
    (passes, figures); measures everything before judging"""
    from parity import floor_report, rel_l2
    B, S = ref["out"].shape[:2]
    vm = torch.zeros(B, S, 1, dtype=torch.float64)
    for i in range(B):
        vm[i, :Li + int(valid[i])] = 1
    tm = vm[:, Li:]
    e = rel_l2(got["out"].double().cpu() * vm, ref["out"] * vm)
    ei, et = rel_l2(got["dimg"], ref["dimg"]), rel_l2(got["dtxt"].double().cpu() * tm, ref["dtxt"] * tm)
    overall, ofloor, worst, bad, ratio, at = floor_report([(n, got["grads"][n], ref["grads"][n]) for n in ref["grads"]], noisy["grads"], 0.98, 0.2)
    ok = e < 1e-2 and ei < 3e-2 and et < 3e-2 and not bad and overall < 1.5 * ofloor
    return ok, dict(fwd=e, dimg=ei, dtxt=et, overall=overall, floor=ofloor, worst=worst, ratio=ratio, at=at, bad=bad)
