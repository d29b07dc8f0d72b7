"""float64 CPU restatement of the temporal attention with relative-position tables (lvdm/modules/attention.py:19-42 RelativePosition,
:126-149 the relative_position branch of CrossAttention.forward), with a hand-written backward -- what csrc/attn_relpos.hip is tested
against.  For one sequence of T rows and one head, idx(i, j) = clamp(j - i, -P, P) + P (key minus query):

    S[i,j] = scale (q_i.k_j + q_i.Ek[idx]),   p = softmax_j S,   o_i = sum_j p[i,j] (v_j + Ev[idx])
    dP = dO (v_j + Ev[idx]),  delta_i = sum_j p dP,  dS = p (dP - delta)
    dV_j = sum_i p dO_i, dEv[t] = sum_{idx=t} p dO_i, dQ_i = scale sum_j dS (k_j + Ek[idx]), dK_j = scale sum_i dS q_i,
    dEk[t] = scale sum_{idx=t} dS q_i           (table gradients summed over all sequences and heads)

`variant` builds the mistakes a kernel is most likely to make; each is a consistent forward + backward of the WRONG function:
    "transposed" i - j instead of j - i;  "no_k" the score term dropped;  "no_v" the output term dropped;
    "unscaled" the table score not multiplied by scale;  "unclamped" index j - i + P, rows outside the table read as zero (T > P only)."""
import math

import torch

VARIANTS = ("exact", "transposed", "no_k", "no_v", "unscaled", "unclamped")
LOG2E = 1.4426950408889634


def rel_index(T: int, P: int, variant: str = "exact"):
    """(idx [T, T] int64 into the table rows, valid [T, T] bool: False where the variant reads a zero instead of a table row)"""
    i = torch.arange(T)[:, None]
    j = torch.arange(T)[None, :]
    d = (i - j) if variant == "transposed" else (j - i)
    if variant == "unclamped":
        raw = d + P
        valid = (raw >= 0) & (raw <= 2 * P)
        return raw.clamp(0, 2 * P), valid
    return d.clamp(-P, P) + P, torch.ones(T, T, dtype=torch.bool)


def relpos_attention(q, k, v, rel_k, rel_v, do, T: int, H: int, scale: float = 0.125, variant: str = "exact"):
    """q, k, v, do: [R, H*64] (R / T consecutive sequences of T rows); rel_k, rel_v: [2P+1, 64].  Returns a dict of float64 tensors:
    o [R, H*64], lse2 [H, R] (base-2 log-sum-exp of the total scaled score), dq, dk, dv [R, H*64], d_rel_k, d_rel_v [2P+1, 64]"""
    assert variant in VARIANTS, variant
    R = q.shape[0]
    assert R % T == 0 and rel_k.shape == rel_v.shape and rel_k.shape[0] % 2 == 1
    P = (rel_k.shape[0] - 1) // 2
    n = R // T
    sp = lambda t: t.double().view(n, T, H, 64).permute(0, 2, 1, 3)                     # [n, H, T, 64]
    mg = lambda t: t.permute(0, 2, 1, 3).reshape(R, H * 64)
    q4, k4, v4, do4 = sp(q), sp(k), sp(v), sp(do)
    idx, valid = rel_index(T, P, variant)
    ek = rel_k.double()[idx] * valid[..., None]                                        # [T, T, 64]
    ev = rel_v.double()[idx] * valid[..., None]
    fk = {"no_k": 0.0, "unscaled": 1.0}.get(variant, scale)                             # factor of the table score
    fv = 0.0 if variant == "no_v" else 1.0
    S = scale * torch.einsum("nhid,nhjd->nhij", q4, k4) + fk * torch.einsum("nhid,ijd->nhij", q4, ek)
    lse = torch.logsumexp(S, -1)
    p = torch.exp(S - lse[..., None])
    o = torch.einsum("nhij,nhjd->nhid", p, v4) + fv * torch.einsum("nhij,ijd->nhid", p, ev)
    # ---- backward ----
    dP = torch.einsum("nhid,nhjd->nhij", do4, v4) + fv * torch.einsum("nhid,ijd->nhij", do4, ev)
    delta = (p * dP).sum(-1, keepdim=True)
    dS = p * (dP - delta)
    dv = torch.einsum("nhij,nhid->nhjd", p, do4)
    dq = scale * torch.einsum("nhij,nhjd->nhid", dS, k4) + fk * torch.einsum("nhij,ijd->nhid", dS, ek)
    dk = scale * torch.einsum("nhij,nhid->nhjd", dS, q4)
    g_ev = fv * torch.einsum("nhij,nhid->ijd", p, do4) * valid[..., None]               # [T, T, 64], per (i, j) pair
    g_ek = fk * torch.einsum("nhij,nhid->ijd", dS, q4) * valid[..., None]
    d_rel_k = torch.zeros(2 * P + 1, 64, dtype=torch.float64).index_add_(0, idx.reshape(-1), g_ek.reshape(T * T, 64))
    d_rel_v = torch.zeros(2 * P + 1, 64, dtype=torch.float64).index_add_(0, idx.reshape(-1), g_ev.reshape(T * T, 64))
    return {"o": mg(o), "lse2": (lse * LOG2E).permute(1, 0, 2).reshape(H, R), "dq": mg(dq), "dk": mg(dk), "dv": mg(dv),
            "d_rel_k": d_rel_k, "d_rel_v": d_rel_v}


def outside(got, ref, rtol: float, atol: float) -> float:
    """share of the elements of got outside atol + rtol |ref| of ref"""
    return ((got - ref).abs() > atol + rtol * ref.abs()).double().mean().item()


# ---- the GPU test's cases and inputs (tests/test_vc1_gpu.py); the CPU suite checks on them that every wrong variant is told apart ----
CASES = [(256, 16, 2, 16), (80, 16, 1, 16), (160, 32, 2, 16), (264, 8, 1, 4), (72, 4, 8, 16), (130, 2, 1, 1), (97, 1, 2, 16)]
BIG_CASE = (40960, 16, 5, 16)
TABLE_SCALE = 0.25          # xavier_uniform_'s bound for a [2P+1, 64] table is about 0.25 (attention.py:26-27)


def case_inputs(R: int, T: int, H: int, P: int):
    """bf16-rounded randn inputs of one case: fused qkv [R, 3 H 64], dO [R, H 64], tables [2P+1, 64] (randn x TABLE_SCALE), as float32"""
    g = torch.Generator().manual_seed(1000 * R + 10 * T + P)
    rb = lambda t: t.to(torch.bfloat16).float()
    D = H * 64
    qkv = rb(torch.randn(R, 3 * D, generator=g))
    do = rb(torch.randn(R, D, generator=g))
    rel_k = rb(torch.randn(2 * P + 1, 64, generator=g) * TABLE_SCALE)
    rel_v = rb(torch.randn(2 * P + 1, 64, generator=g) * TABLE_SCALE)
    return qkv, do, rel_k, rel_v


def case_reference(R: int, T: int, H: int, P: int, variant: str = "exact"):
    qkv, do, rel_k, rel_v = case_inputs(R, T, H, P)
    D = H * 64
    return relpos_attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], rel_k, rel_v, do, T, H, 0.125, variant)


# ---------------------------------------------------------------------------------------------------------------------
# the VideoCrafter1 layout of the UNet (use_relative_position=True, temporal_conv=False): configuration, seeded weights and a CPU
# restatement built on oracle/unet_oracle.py (its CrossAttention swapped for the one with the two tables while the forward runs)
# ---------------------------------------------------------------------------------------------------------------------
def vc1_tiny_config():
    """make_golden_unet.py's tiny configuration without the temporal convolutions (temporal_length 4: tables [9, 64])"""
    import unet_oracle as U
    return U.tiny_config(temporal_conv=False)


def vc1_table_names(cfg):
    """the table names of a relative-position net (four per temporal transformer), in the reference's registration order"""
    return [n for n in vc1_param_shapes(cfg) if n.endswith(".embeddings_table")]


def vc1_param_shapes(cfg):
    """{name: shape} in the order of the reference module's named_parameters(): unet_oracle's list with the two tables of every
    temporal CrossAttention right after its to_out.0.bias (attention.py:87-95)"""
    import unet_oracle as U
    st = U.structure(cfg)
    layers = [l for blk in st["input"] for l in blk] + ([st["init_attn"]] if st["init_attn"] is not None else []) + list(st["middle"]) \
        + [l for blk in st["output"] for l in blk]
    after = {f"{pre}.transformer_blocks.0.{a}.to_out.0.bias": f"{pre}.transformer_blocks.0.{a}"
             for kind, pre, _ in layers if kind == "tt" for a in ("attn1", "attn2")}
    out = {}
    for n, s in U.param_shapes(cfg).items():
        out[n] = s
        if n in after:
            for t in ("relative_position_k", "relative_position_v"):
                out[f"{after[n]}.{t}.embeddings_table"] = (2 * cfg.temporal_length + 1, cfg.num_head_channels)
    assert len(after) and sum(n.endswith(".embeddings_table") for n in out) == 2 * len(after)
    return out


def vc1_init_params(cfg, seed: int = 0, dtype=torch.float32):
    """unet_oracle.init_params' rule (nothing left at zero) with the tables drawn randn x TABLE_SCALE"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, s in vc1_param_shapes(cfg).items():
        if k.endswith(".embeddings_table"):
            w = torch.randn(s, generator=g) * TABLE_SCALE
        elif len(s) == 1:
            w = torch.randn(s, generator=g) * 0.1 + (1.0 if k.endswith("weight") else 0.0)
        else:
            w = torch.randn(s, generator=g) * (0.7 / math.sqrt(math.prod(s[1:])))
        out[k] = w.to(dtype)
    return out


def relpos_cross_attention(x, P, pre, heads, context=None, text_len=77):
    """unet_oracle.cross_attention with the relative_position branch of CrossAttention.forward (attention.py:126-149) where P holds the
    tables of `pre`; autograd does the backward, in whatever dtype the inputs have"""
    import torch.nn.functional as F
    import unet_oracle as U
    tk = P.get(pre + ".relative_position_k.embeddings_table")
    if tk is None:
        return _ORIGINAL["cross_attention"](x, P, pre, heads, context, text_len)
    assert context is None, "the reference enables relative positions on temporal self-attention only"
    tv = P[pre + ".relative_position_v.embeddings_table"]
    q, k, v = (U.lora_linear(x, P, pre + n) for n in (".to_q", ".to_k", ".to_v"))
    B, N, C = q.shape
    d = C // heads
    sp = lambda t: t.reshape(B, N, heads, d).permute(0, 2, 1, 3)
    q, k, v = sp(q), sp(k), sp(v)
    idx, _ = rel_index(N, (tk.shape[0] - 1) // 2)
    sim = (torch.einsum("bhid,bhjd->bhij", q, k) + torch.einsum("bhtd,tsd->bhts", q, tk[idx])) * (d ** -0.5)
    p = sim.softmax(dim=-1)
    o = torch.einsum("bhij,bhjd->bhid", p, v) + torch.einsum("bhts,tsd->bhtd", p, tv[idx])
    o = o.permute(0, 2, 1, 3).reshape(B, N, C)
    return F.linear(o, P[pre + ".to_out.0.weight"], P[pre + ".to_out.0.bias"])


_ORIGINAL = {}


def vc1_unet_forward(P, cfg, x, timesteps, context, fps=16):
    """unet_oracle.unet_forward of a parameter dict that holds relative-position tables"""
    import unet_oracle as U
    _ORIGINAL["cross_attention"] = U.cross_attention
    U.cross_attention = relpos_cross_attention
    try:
        return U.unet_forward(P, cfg, x, timesteps, context, fps=fps)
    finally:
        U.cross_attention = _ORIGINAL["cross_attention"]
