"""Ill-conditioned inputs for the normalisation and attention kernels, and CPU restatements of the two policies they aim at.

Every other parity test draws `randn`: mean near 0, standard deviation near 1.  Two code paths never see anything else:
  * GroupNorm's statistics (csrc/groupnorm.hip).  A one-pass `E[x^2] - mean^2` in fp32 loses the variance once |mean| >> std; the builders
    here put the mean 30 .. 800 standard deviations away from zero, as a bias-dominated convolution in front of a static or letterboxed
    clip does.
  * the lazy running maximum of the flash-attention forwards (csrc/attn128.hip, attn_fwd.hip, attn_gen.hip): the reference moves, and the
    accumulators are rescaled, only when a tile's maximum outgrows it by more than 8 log2 units.  With randn q / k at scale = d^-1/2 that
    never happens after the first key tile; the builders scale single keys so that it does, in every tile position.
Pure torch / numpy, no GPU: the CPU and the GPU tests draw identical tensors from a seed."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

BF = torch.bfloat16
LOG2E = 1.4426950408889634


def rb(t):
    return t.to(BF).float()


# ------------------------------------------------------------------------------------------------ GroupNorm inputs
GN_CASES = ("dc_offset", "plateau", "plateau_small", "constant_group", "outlier_channel", "two_samples")
GN_ILL = ("dc_offset", "plateau", "plateau_small")                    # a one-pass fp32 variance must miss the statistic bar on these
GN_SHAPES = ((4096, 64, 8), (1024, 320, 32), (64, 2560, 32))          # P, C, G: 8 | 10 | 80 channels per group; one | one | two channel passes
GN_STAT_RTOL = 1e-4                                                   # the LayerNorm statistic bar (test_kernels_gpu._ln_modulate_case)
GN_STAT_ATOL_MEAN = 1e-4                                              # ... whose absolute part matters for means near zero only


def _plateau(shape, level, step, gen):
    """`level` everywhere, 1 % of the elements raised by `step` (both exact in bf16)"""
    return level + step * (torch.rand(shape, generator=gen) < 0.01).float()


@functools.lru_cache(maxsize=None)
def gn_case(name, P, C, G):
    """-> dict(x [N,P,C], gamma [C], beta [C], dy [N,P,C], G, eps, silu); every tensor fp32 holding bf16-representable values"""
    gen = torch.Generator().manual_seed(1000 * GN_CASES.index(name) + P + C)
    cpg = C // G
    N = 2 if name == "two_samples" else 1
    if name == "dc_offset":
        x = 128 + torch.randn(N, P, C, generator=gen)
    elif name == "plateau":
        x = _plateau((N, P, C), 100.0, 0.5, gen)
    elif name == "plateau_small":
        x = _plateau((N, P, C), 20.0, 0.125, gen)
    elif name == "constant_group":
        x = torch.randn(N, P, C, generator=gen)
        x[:, :, cpg:2 * cpg] = 3.140625
    elif name == "outlier_channel":
        x = torch.randn(N, P, C, generator=gen)
        for g in range(G):
            c = g * cpg + g % cpg
            x[:, :, c] = 200 + torch.randn(N, P, generator=gen)
    elif name == "two_samples":
        x = torch.cat([_plateau((1, P, C), 100.0, 0.5, gen), torch.randn(1, P, C, generator=gen)], 0)
    else:
        raise KeyError(name)
    gamma = rb(1 + 0.2 * torch.randn(C, generator=gen))
    beta = rb(0.2 * torch.randn(C, generator=gen))
    dy = rb(torch.randn(N, P, C, generator=gen))
    return dict(x=rb(x), gamma=gamma, beta=beta, dy=dy, G=G, eps=1e-6, silu=name != "outlier_channel")


@functools.lru_cache(maxsize=None)
def gn_reference(name, P, C, G):
    """fp64: y, mean [N,G], rstd [N,G], dx, dgamma, dbeta of F.group_norm (+ SiLU) on gn_case(name, P, C, G).  Computed once and shared."""
    c = gn_case(name, P, C, G)
    x = c["x"].double().requires_grad_(True)
    ga = c["gamma"].double().requires_grad_(True); be = c["beta"].double().requires_grad_(True)
    y = F.group_norm(x.permute(0, 2, 1), G, ga, be, c["eps"]).permute(0, 2, 1)
    if c["silu"]:
        y = F.silu(y)
    (y * c["dy"].double()).sum().backward()
    N = x.shape[0]
    xg = x.detach().view(N, P, G, C // G).permute(0, 2, 1, 3).reshape(N, G, -1)
    mean = xg.mean(-1)
    var = ((xg - mean[..., None]) ** 2).mean(-1)                       # two-pass in fp64: the truth
    return dict(y=y.detach(), mean=mean, var=var, rstd=1.0 / (var + c["eps"]).sqrt(), dx=x.grad, dgamma=ga.grad, dbeta=be.grad)


# ------------------------------------------------------------------------------------------------ GroupNorm fp32 restatements
def gn_slabs(N, P, C):
    """the position slabs and thread rows of gn_stats_kernel's launch (csrc/groupnorm.hip)"""
    nch = C >> 3
    rows = 1 if nch >= 256 else 256 // nch
    want = min((384 + N - 1) // N, P // (4 * rows))
    return max(1, min(2048, want)), rows


def _kernel_order_sums(v, N):
    """v: [P, C] fp32 -> per-channel fp32 sums in the kernel's order: a thread adds the positions p0 + row, p0 + row + rows, ... of its slab
    serially, then the thread partials of a slab and the slab totals are added one after the other (the atomics' order is not fixed on
    the device; any order of a few hundred partials carries the same error)"""
    P, C = v.shape
    slabs, rows = gn_slabs(N, P, C)
    total = np.zeros(C, np.float32)
    for s in range(slabs):
        p0, p1 = P * s // slabs, P * (s + 1) // slabs
        blk = v[p0:p1]
        pad = (-len(blk)) % rows
        if pad:
            blk = np.concatenate([blk, np.zeros((pad, C), np.float32)], 0)
        part = np.add.accumulate(blk.reshape(-1, rows, C), axis=0, dtype=np.float32)[-1]           # [rows, C], serial in fp32
        total = (total + np.add.accumulate(part, axis=0, dtype=np.float32)[-1]).astype(np.float32)
    return total


def gn_stats_naive_fp32(x, G, eps):
    """the one-pass statistics: per-channel sums of x and x^2 in fp32, folded into groups, var = max(E[x^2] - mean^2, 0).
    x [N,P,C] fp32 -> (mean [N,G], rstd [N,G]) as fp32 numpy arrays"""
    N, P, C = x.shape
    cpg = C // G
    mean = np.zeros((N, G), np.float32); rstd = np.zeros((N, G), np.float32)
    for n in range(N):
        v = x[n].numpy().astype(np.float32)
        s = _kernel_order_sums(v, N); q = _kernel_order_sums(v * v, N)
        cnt = np.float32(cpg) * np.float32(P)
        for g in range(G):
            sg = np.add.accumulate(s[g * cpg:(g + 1) * cpg], dtype=np.float32)[-1]
            qg = np.add.accumulate(q[g * cpg:(g + 1) * cpg], dtype=np.float32)[-1]
            m = np.float32(sg / cnt)
            var = max(np.float32(np.float32(qg / cnt) - np.float32(m * m)), np.float32(0))
            mean[n, g] = m; rstd[n, g] = np.float32(1) / np.sqrt(np.float32(var + np.float32(eps)))
    return mean, rstd


def gn_stats_shifted_fp32(x, G, eps):
    """the same single pass about a per-channel pivot k_c = x[n, 0, c]: sums of (x - k_c) and (x - k_c)^2 in fp32, per-channel
    M2_c = q_c - s_c^2 / P, and the parallel-variance fold  M2_g = sum_c M2_c + P sum_c (mean_c - mean_g)^2  with the channel means taken
    relative to the group's first pivot.  Everything in fp32."""
    N, P, C = x.shape
    cpg = C // G
    f = np.float32
    mean = np.zeros((N, G), np.float32); rstd = np.zeros((N, G), np.float32)
    for n in range(N):
        v = x[n].numpy().astype(np.float32)
        k = v[0].copy()
        d = (v - k[None, :]).astype(np.float32)
        s = _kernel_order_sums(d, N); q = _kernel_order_sums((d * d).astype(np.float32), N)
        invp = f(1) / f(P)
        for g in range(G):
            sl = slice(g * cpg, (g + 1) * cpg)
            dc = ((k[sl] - k[g * cpg]).astype(np.float32) + (s[sl] * invp).astype(np.float32)).astype(np.float32)   # mean_c - k_g
            m2c = np.maximum((q[sl] - (s[sl] * s[sl]).astype(np.float32) * invp).astype(np.float32), f(0))
            dg = f(np.add.accumulate(dc, dtype=np.float32)[-1] / f(cpg))                                            # mean_g - k_g
            dev = (dc - dg).astype(np.float32)
            m2 = f(np.add.accumulate(m2c, dtype=np.float32)[-1]) + f(P) * f(np.add.accumulate((dev * dev).astype(np.float32), dtype=np.float32)[-1])
            var = f(m2 / (f(cpg) * f(P)))
            mean[n, g] = f(k[g * cpg] + dg); rstd[n, g] = f(1) / np.sqrt(f(var + f(eps)))
    return mean, rstd


def stat_miss(got, ref, rtol, atol=0.0):
    """the largest excess of |got - ref| over atol + rtol |ref|, as a multiple of that tolerance (<= 1: within the bar)"""
    got = torch.as_tensor(np.asarray(got, np.float64)); ref = ref.double()
    return ((got - ref).abs() / (atol + rtol * ref.abs())).max().item()


# ------------------------------------------------------------------------------------------------ softmax inputs
SOFTMAX_CASES = ("late_spike", "staircase", "weak_first_tile")


def scale_keys(k, name, mult=1.0):
    """k: a key tensor whose dim 1 is the key index (any trailing dims).  Scales whole key rows in place, returns k.
      late_spike       key S-3 x 12 and key S//2 x 6: one rescale late in the loop, one in the middle; with kv_len = S - 33 the x 12 key is masked
      staircase        key 64 t + 17 x 3 (t + 1) in every 64-key tile t: the maximum climbs tile after tile
      weak_first_tile  keys 0..63 x 0.05, the rest x 3: the reference set by tile 0 is far too low for everything after it
    mult scales the factors (the CPU tests' saturating rows)."""
    S = k.shape[1]
    if name == "late_spike":
        k[:, S - 3] *= 12.0 * mult
        k[:, S // 2] *= 6.0 * mult
    elif name == "staircase":
        for t in range((S + 63) // 64):
            if 64 * t + 17 < S:
                k[:, 64 * t + 17] *= 3.0 * (t + 1) * mult
    elif name == "weak_first_tile":
        k[:, :64] *= 0.05
        k[:, 64:] *= 3.0 * mult
    elif name == "masked_giant":
        # only meant for kv_len = S - 33: key S - 32 lies behind the mask but inside the last key tile the kernels still load (late_spike's
        # key S - 3 is in a tile they never visit).  Were its score to move the running reference, every valid key's exp2 would fall below
        # the smallest fp32 (a reference moved by a x 12 key is still within range and is divided out again)
        k[:, S - 32] *= 150.0 * mult
    elif name != "randn":
        raise KeyError(name)
    return k


def softmax_qkv(name, B, S, H, hd=128, mult=1.0):
    """-> bf16 [B, S, 3 * H * hd], the fused q | k | v rows the head_dim-128 kernels consume in place"""
    gen = torch.Generator().manual_seed(S + H + 7 * (["randn"] + list(SOFTMAX_CASES) + ["masked_giant"]).index(name))
    qkv = torch.randn(B, S, 3, H, hd, generator=gen)
    scale_keys(qkv[:, :, 1], name, mult)
    return qkv.reshape(B, S, 3 * H * hd).to(BF)


def dense_attention64(qkv, H, kv_len=None, g=None):
    """fp64 dense attention on fused rows [B, S, 3 H hd]: (o [B,S,H hd], lse2 [B,H,S], s [B,H,S,S], d qkv or None)"""
    B, S, C3 = qkv.shape
    C = C3 // 3
    hd = C // H
    x = qkv.double().requires_grad_(g is not None)
    qr, kr, vr = [t.reshape(B, S, H, hd) for t in x.split(C, dim=-1)]
    s = torch.einsum("bqhd,bkhd->bhqk", qr, kr) * hd ** -0.5
    if kv_len is not None:
        dead = torch.arange(S)[None, :] >= torch.as_tensor(kv_len)[:, None].long()
        s = s.masked_fill(dead[:, None, None, :], float("-inf"))
    o = torch.einsum("bhqk,bkhd->bqhd", s.softmax(-1), vr).reshape(B, S, C)
    if g is not None:
        o.backward(g.double())
    return o.detach(), torch.logsumexp(s.detach(), -1) * LOG2E, s.detach(), (x.grad if g is not None else None)


# ------------------------------------------------------------------------------------------------ the lazy-maximum policy, restated
LAZY_THRESHOLD = 8.0          # log2 units (attn128.hip: `mxs - m_run <= 8.0f`)
_NEG = -1.0e30


def lazy_max_coverage(qkv, H, kv_len=None, tile=64, wave_rows=32):
    """attn128_fwd's reference policy in fp64, per (sample, head) and per wave of 32 query rows (rows past S repeat row S - 1):
    a key tile's scores split over the two lane halves of a query (keys with key % 8 < 4 | >= 4); the wave takes the rescale branch at
    tile 0 and whenever ANY half of ANY of its rows sees a maximum more than 8 above its running reference; then both halves of every row
    move to max(reference, tile maximum).  Masked keys (>= kv_len) score -1e30 and move nothing.
    -> dict(rows, rescaled: rows whose reference moved at a tile > 0, stale: rows that at some tile > 0 kept a reference below the tile's
    maximum (rise in (0, 8]), max_rise: the largest such rise)"""
    B, S, C3 = qkv.shape
    C = C3 // 3
    hd = C // H
    x = qkv.double()
    q, k = [t.reshape(B, S, H, hd) for t in x.split(C, dim=-1)[:2]]
    s_all = torch.einsum("bqhd,bkhd->bhqk", q, k) * (hd ** -0.5 * LOG2E)
    rescaled = stale = 0
    max_rise = 0.0
    for b in range(B):
        klen = S if kv_len is None else min(int(kv_len[b]), S)
        nt = (klen + tile - 1) // tile
        for h in range(H):
            s = s_all[b, h].clone()
            s[:, klen:] = _NEG
            s = F.pad(s, (0, nt * tile - S), value=_NEG) if nt * tile > S else s[:, :nt * tile]
            half = (torch.arange(nt * tile) % 8) // 4
            for w0 in range(0, S, wave_rows):
                rows = torch.arange(w0, w0 + wave_rows).clamp_max(S - 1)
                live = torch.arange(w0, w0 + wave_rows) < S
                m_run = torch.full((wave_rows,), _NEG, dtype=torch.float64)
                resc = torch.zeros(wave_rows, dtype=torch.bool); stl = torch.zeros(wave_rows, dtype=torch.bool)
                for t in range(nt):
                    st = s[rows, t * tile:(t + 1) * tile]
                    hf = half[t * tile:(t + 1) * tile]
                    mxh = torch.stack([st[:, hf == 0].max(1).values, st[:, hf == 1].max(1).values], 1)       # [rows, 2]
                    mx = mxh.max(1).values
                    if t == 0 or bool(((mxh - m_run[:, None]) > LAZY_THRESHOLD).any()):
                        m_new = torch.maximum(m_run, mx)
                        if t > 0:
                            resc |= m_new > m_run
                        m_run = m_new
                    rise = mx - m_run
                    if t > 0:
                        stl |= (rise > 0) & (rise <= LAZY_THRESHOLD)
                        if bool(((rise > 0) & live).any()):
                            max_rise = max(max_rise, rise[live].max().item())
                    assert bool((rise <= LAZY_THRESHOLD).all())
                rescaled += int((resc & live).sum()); stale += int((stl & live).sum())
    return dict(rows=B * H * S, rescaled=rescaled, stale=stale, max_rise=max_rise)


# ------------------------------------------------------------------------------------------------ LayerNorm-family rows
LN_ROWS = ("dc_offset", "one_huge", "constant")


def ln_rows(kind, M, D, gen):
    """[M, D] fp32, bf16-representable: every row `100 + randn`; randn rows with one element 1000 x the rest; rows that are one constant
    each (a different one per row)"""
    if kind == "dc_offset":
        x = 100 + torch.randn(M, D, generator=gen)
    elif kind == "one_huge":
        x = torch.randn(M, D, generator=gen)
        at = torch.randint(0, D, (M,), generator=gen)
        x[torch.arange(M), at] *= 1000.0
    elif kind == "constant":
        x = (torch.randn(M, 1, generator=gen) * 3).expand(M, D).clone()
    else:
        raise KeyError(kind)
    return rb(x)


def saturated_rows(s, nats=100.0):
    """s: scores [..., q, k] (nats, -inf where masked) -> bool [..., q]: the best key leads the second best by more than `nats`"""
    top = s.topk(2, dim=-1).values
    return (top[..., 0] - top[..., 1]) > nats


def finite(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts if t is not None)


assert math.isclose(LOG2E, 1 / math.log(2))
